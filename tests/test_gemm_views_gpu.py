"""GPU: every GEMM route on framed views, against the float64 reference, exactly (tests/gemm_cases.py).

One case per test: the frames are built, the library's route report for the real pointers must equal the route the case
expects, the call is launched once through polus_amd.ops with the case's switches, and the shared comparator checks the
outputs (== on the exact cases), their finiteness and every byte of the output allocations outside the views.  A fast-route
case with a non-dense view is also compared bit for bit with its all-dense twin."""
import numpy as np
import pytest
import torch

from tests import gemm_cases as gc
from tests.gemm_cases import CASES, DT, GUARD, build, check, expected_route, reference, switches

pytestmark = pytest.mark.gpu


def device_frames(frames):
    """name -> (the whole allocation on the device, the view handed to the library)."""
    out = {}
    for n, fr in frames.items():
        t = torch.from_numpy(fr.buf).to(DT[fr.dtype]).cuda()
        assert t.data_ptr() % 256 == 0
        v = t[GUARD:GUARD + fr.rows, fr.c0:fr.c0 + fr.cols]
        out[n] = (t, v[0] if fr.vector else v)
    return out


def launch(case, d, route_only=False):
    """The case's call on the views of d; route_only: its route report instead."""
    from polus_amd import ops
    v = {n: view for n, (_, view) in d.items()}
    if case.op == "gemm":
        f = ops.gemm_route if route_only else ops.gemm
        return f(v["A"], v["B"], v["C"], bias=v.get("bias"), resid=v.get("resid"), aux=v.get("aux"), **gc.gemm_keywords(case))
    if case.op == "dw":
        f = ops.dense_bwd_params_route if route_only else ops.dense_bwd_params
        return f(v["dY"], v["X"], v["dW"], v.get("db"), accumulate=case.accumulate, split_k=case.split_k)
    if case.op == "dwg":
        f = ops.dense_bwd_params_grouped_route if route_only else ops.dense_bwd_params_grouped
        probs = [(v[f"dY{k}"], v[f"X{k}"], v[f"dW{k}"], v.get(f"db{k}")) for k in range(len(case.shape[1]))]
        return f(probs, accumulate=case.accumulate, split_k=case.split_k)
    if route_only:
        return None
    if case.op == "thin_fwd":
        return ops.dense_thin_fwd(v["x"], v["w"], v["bias"], v["y"])
    return ops.dense_thin_bwd(v["x"], v["dy"], v["w"], v["dx"], v["dw"], v.get("db"), accumulate=case.accumulate)


def run(case):
    """Launches the case once; returns (frames, frames_after of the outputs, the route report)."""
    from polus_amd._lib import PolusHipError
    frames = build(case)
    d = device_frames(frames)
    with switches(case):
        route = launch(case, d, route_only=True)
        if case.refused:
            with pytest.raises(PolusHipError):
                launch(case, d)
        else:
            launch(case, d)
    torch.cuda.synchronize()
    after = {n: d[n][0].float().cpu().numpy() for n in gc.outputs(case, frames)}
    return frames, after, route


_TWINS = {}


def twin_views(case):
    """The output views of the all-dense twin, launched once per base."""
    if case.base not in _TWINS:
        twin = gc.dense_twin(case)
        frames, after, _ = run(twin)
        _TWINS[case.base] = {n: frames[n].view_of(a).copy() for n, a in after.items()}
    return _TWINS[case.base]


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_gemm_case(name):
    case = gc.BY_NAME[name]
    frames, after, route = run(case)
    if route is not None:
        want = expected_route(case, frames)
        got = route._asdict()
        assert got == want, (got, want)
    findings = check(case, after, None if case.refused else reference(case, frames))
    assert not findings, "\n".join(findings)
    if case.fast and case.views and case.exact:
        for n, dense in twin_views(case).items():
            got = frames[n].view_of(after[n])
            assert np.array_equal(got.view(np.uint32), dense.view(np.uint32)), f"{n}: differs from the all-dense launch"
