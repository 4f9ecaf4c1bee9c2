"""CPU: the one forwarding rule of the model shells (polus_amd.models.ModelShell) and the one buffer cache
(polus_amd.tensor.cached_buffer), over stub inner models: the real ones allocate their arena on the GPU
(tests/test_model_state_gpu.py runs the same reads on them)."""
import ast
import inspect
import textwrap

import pytest
import torch

from polus_amd import graph
from polus_amd.models import STEP_STATE, BertForMaskedLM, ModelShell
from polus_amd.tensor import cached_buffer


class Inner:
    """What a shell needs of the model inside it: the attributes BertModel declares in its initialiser."""
    arena = config = compute_dtype = None

    def __init__(self):
        self.grad_ready_hook, self.deterministic = None, False
        self.dropout_step, self.overlap_dw = 0, True
        self.graph_seeds = self.identical_dropout_across_ranks = False

    def site_seed(self, layer, site, step=None):
        return (layer, site, step, self.dropout_step, self.graph_seeds)


def _chain(levels):
    inner = Inner()
    outer = inner
    for _ in range(levels):
        outer = ModelShell(outer)
    return outer, inner


VALUES = {"dropout_step": 7, "overlap_dw": False, "graph_seeds": True, "deterministic": True,
          "identical_dropout_across_ranks": True}


def test_the_values_cover_the_tuple_and_differ_from_the_defaults():
    assert set(VALUES) == set(STEP_STATE)
    fresh = Inner()
    assert all(getattr(fresh, n) != VALUES[n] for n in STEP_STATE)


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("name", STEP_STATE)
def test_step_state_is_the_innermost_models(name, levels):
    outer, inner = _chain(levels)
    default = getattr(inner, name)
    assert getattr(outer, name) == default           # building the shells moved nothing
    setattr(outer, name, VALUES[name])
    assert getattr(inner, name) == VALUES[name]
    setattr(inner, name, default)
    assert getattr(outer, name) == default
    node = outer
    while node is not inner:                         # no shell keeps a copy of its own
        assert name not in vars(node)
        node = node.inner


@pytest.mark.parametrize("levels", [1, 2])
def test_hook_and_reads_go_through(levels):
    outer, inner = _chain(levels)
    hook = lambda lo, hi, variables: None
    outer.grad_ready_hook = hook
    assert inner.grad_ready_hook is hook
    outer.grad_ready_hook = None
    assert inner.grad_ready_hook is None and outer.grad_ready_hook is None
    inner.grad_ready_hook = hook
    assert outer.grad_ready_hook is hook
    assert getattr(outer, "tokens_per_step", None) is None       # before the first call, as training.py asks
    inner.tokens_per_step, inner._shape = 48, (3, 16)
    assert outer.tokens_per_step == 48 and outer._shape == (3, 16)
    outer.dropout_step, outer.graph_seeds = 5, True
    assert outer.site_seed(0, 1) == inner.site_seed(0, 1) == (0, 1, None, 5, True)
    assert outer.site_seed(-1, 0, 9) == (-1, 0, 9, 5, True)


def test_a_new_shell_resets_what_the_base_initialiser_assigns_and_nothing_else():
    inner = Inner()
    inner.dropout_step, inner.overlap_dw = 3, False
    ModelShell(inner)
    assert (inner.dropout_step, inner.overlap_dw, inner.deterministic, inner.grad_ready_hook) == (3, False, False, None)


def _assigned_on_model(func):
    """Names `func` assigns as `model.<name> = ...` or `model.<name> += ...`, tuple targets included."""
    names = set()
    for node in ast.walk(ast.parse(textwrap.dedent(inspect.getsource(func)))):
        targets = node.targets if isinstance(node, ast.Assign) else [node.target] if isinstance(node, ast.AugAssign) else []
        for t in targets:
            for leaf in ast.walk(t):
                if isinstance(leaf, ast.Attribute) and isinstance(leaf.value, ast.Name) and leaf.value.id == "model":
                    names.add(leaf.attr)
    return names


def test_the_tuple_holds_what_the_step_graph_sets_on_the_model():
    found = _assigned_on_model(graph.GraphedStep._capture) | _assigned_on_model(graph.GraphedStep.__call__)
    assert found >= {"overlap_dw", "graph_seeds", "dropout_step"}, found      # the walk sees the assignments at all
    assert found <= set(STEP_STATE), found - set(STEP_STATE)


def test_the_shells_define_none_of_the_forwarded_names_themselves():
    from polus_amd.ir.models import CrossEncoder, SpladeEncoder
    for cls in (BertForMaskedLM, SpladeEncoder, CrossEncoder):
        assert issubclass(cls, ModelShell)
        own = set(vars(cls)) & (set(STEP_STATE) | {"grad_ready_hook", "site_seed", "tokens_per_step", "_shape", "_buf"})
        assert not own, (cls.__name__, own)


def test_cached_buffer():
    cache = {}
    a = cached_buffer(cache, "x", (3, 4), torch.float32, "cpu")
    assert tuple(a.shape) == (3, 4) and a.dtype == torch.float32 and a.device.type == "cpu"
    assert cached_buffer(cache, "x", (3, 4), torch.float32, "cpu") is a
    assert cached_buffer(cache, "x", [3, 4], torch.float32, "cpu") is a           # a list or a torch.Size is the same shape
    assert cached_buffer(cache, "x", a.shape, torch.float32, "cpu") is a
    b = cached_buffer(cache, "x", (3, 5), torch.float32, "cpu")
    assert b is not a and tuple(b.shape) == (3, 5) and cache == {"x": b}
    c = cached_buffer(cache, "x", (3, 5), torch.int32, "cpu")
    assert c is not b and c.dtype == torch.int32 and list(cache) == ["x"] and cache["x"] is c
    d = cached_buffer(cache, "y", (3, 5), torch.int32, "cpu")
    assert d is not c and cache["x"] is c and cache["y"] is d and len(cache) == 2
