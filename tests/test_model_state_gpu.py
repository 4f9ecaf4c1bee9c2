"""GPU: the step state set on a model shell is the state of the BertModel at the bottom of it (polus_amd.models.ModelShell),
and masked-LM training replayed from a step graph equals the eager run bit for bit -- which it can only do when
`overlap_dw` and `graph_seeds`, set by GraphedStep on the BertForMaskedLM it holds, reach the encoder inside."""
import pytest
import torch

from tests import mlm_ref as mr
from tests.test_mlm_gpu import TINY, _model, _x
from tests.test_model_state_cpu import VALUES

pytestmark = pytest.mark.gpu


def _shells(mode="f32"):
    from polus_amd.ir.models import CrossEncoder, SpladeEncoder
    from polus_amd.models import BertConfig, BertForMaskedLM
    mlm = BertForMaskedLM(BertConfig(*TINY), compute_dtype=mode)
    inside = BertForMaskedLM(BertConfig(*TINY), compute_dtype=mode)
    cross = CrossEncoder(BertConfig(*TINY), compute_dtype=mode)
    return [(mlm, mlm.bert), (SpladeEncoder(inside), inside.bert), (cross, cross.bert)]


def test_step_state_set_on_a_shell_is_held_by_the_bert_model():
    from polus_amd.models import STEP_STATE, BertModel, dropout_seed, dropout_seed_static
    for shell, bert in _shells():
        what = type(shell).__name__
        assert type(bert) is BertModel
        for name in STEP_STATE:
            default = getattr(bert, name)
            value = (not default) if isinstance(default, bool) else VALUES[name]      # POLUS_OVERLAP_DW may have set one
            assert value != default and getattr(shell, name) == default, (what, name)
            setattr(shell, name, value)
            assert getattr(bert, name) == value, (what, name)
            setattr(bert, name, default)
            assert getattr(shell, name) == default, (what, name)
        hook = lambda lo, hi, variables: None
        shell.grad_ready_hook = hook
        assert bert.grad_ready_hook is hook
        shell.grad_ready_hook = None
        assert bert.grad_ready_hook is None
        shell.dropout_step = 5
        base = bert.dropout_base_seed
        for on in (False, True):
            shell.graph_seeds = on
            want = dropout_seed_static(base, 0, 1) if on else dropout_seed(base, 5, 0, 1)
            assert shell.site_seed(0, 1) == bert.site_seed(0, 1) == want, (what, on)
        assert dropout_seed_static(base, 0, 1) != dropout_seed(base, 5, 0, 1)


def _train(mode, graph, steps=4):
    from polus_amd.losses import MaskedSparseCategoricalCrossentropy
    from polus_amd.optimizers import AdamWeightDecay
    from polus_amd.training import ClassifierTrainer
    model, ocfg, _ = _model(mode, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    model.deterministic = True
    t = ClassifierTrainer(model, AdamWeightDecay(learning_rate=1e-3, weight_decay_rate=0.01), MaskedSparseCategoricalCrossentropy())
    if graph:
        t.enable_step_graph(warmup=1)
    losses = [float(t.train_step(*_x(mr.mlm_batch(ocfg, 3, 16, 4, 70 + s)))) for s in range(steps)]
    torch.cuda.synchronize()
    assert t.optimizer.iterations == steps and model.dropout_step == steps
    return t, losses, model.arena.params.clone()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_masked_lm_training_under_the_step_graph_equals_eager_steps_bitwise(mode):
    """Four steps, the first eager in both runs (warmup=1), so three replays with three dropout salts."""
    _, losses, params = _train(mode, graph=False)
    tg, losses_g, params_g = _train(mode, graph=True)
    print(f"[model state] masked-LM {mode}: eager losses {losses}, graphed {losses_g}")
    assert tg._graphed.graph is not None, "the step was not captured"
    assert losses == losses_g and torch.equal(params, params_g), "the replayed step graph differs from eager steps"
