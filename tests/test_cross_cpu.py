"""CPU: the cross-encoder's checkpoint import (names and shapes against the HF state dict that wrote the file) and the
host-side candidate checks of CrossEncoderIndex."""
import json

import numpy as np
import pytest
import torch


def _save_hf(tmp_path, num_labels=1, pooler=True):
    from safetensors.numpy import save_file
    from transformers import BertConfig, BertForSequenceClassification
    hc = BertConfig(vocab_size=60, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                    max_position_embeddings=32, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, pad_token_id=None,
                    num_labels=num_labels)
    torch.manual_seed(5)
    m = BertForSequenceClassification(hc).eval()
    sd = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()
          if "position_ids" not in k and (pooler or "pooler" not in k)}
    save_file(sd, str(tmp_path / "model.safetensors"))
    json.dump(hc.to_dict(), open(tmp_path / "config.json", "w"), default=str)
    return sd


def test_cross_encoder_checkpoint_mapping(tmp_path):
    from polus_amd.checkpoint import read_local_cross_encoder
    sd = _save_hf(tmp_path)
    cfg, p = read_local_cross_encoder(str(tmp_path))
    assert cfg["hidden_size"] == 128 and cfg["num_hidden_layers"] == 2
    assert np.array_equal(p["classifier.w"], sd["classifier.weight"]) and p["classifier.w"].shape == (1, 128)
    assert np.array_equal(p["classifier.b"], sd["classifier.bias"])
    assert np.array_equal(p["pooler.w"], sd["bert.pooler.dense.weight"])
    assert np.array_equal(p["pooler.b"], sd["bert.pooler.dense.bias"])
    assert np.array_equal(p["emb.word"], sd["bert.embeddings.word_embeddings.weight"])
    assert np.array_equal(p["emb.type"], sd["bert.embeddings.token_type_embeddings.weight"])
    for i in range(2):
        q = f"bert.encoder.layer.{i}.attention.self."
        assert np.array_equal(p[f"layer{i}.qkv.w"], np.concatenate([sd[q + n + ".weight"] for n in ("query", "key", "value")], 0))
        assert np.array_equal(p[f"layer{i}.ffn2.w"], sd[f"bert.encoder.layer.{i}.output.dense.weight"])
        assert np.array_equal(p[f"layer{i}.ln1.g"], sd[f"bert.encoder.layer.{i}.attention.output.LayerNorm.weight"])
    assert "head.w" not in p
    # every tensor of the state dict went somewhere: the element counts agree
    assert sum(v.size for v in p.values()) == sum(v.size for v in sd.values())


def test_cross_encoder_checkpoint_refusals(tmp_path):
    from polus_amd.checkpoint import load_cross_encoder_from_local, read_local_cross_encoder
    with pytest.raises(FileNotFoundError):
        load_cross_encoder_from_local("cross-encoder/ms-marco-MiniLM-L-6-v2")          # by name: refused
    a, b = tmp_path / "two_labels", tmp_path / "no_pooler"
    a.mkdir(); b.mkdir()
    _save_hf(a, num_labels=2)
    with pytest.raises(ValueError, match="num_labels"):
        read_local_cross_encoder(str(a))
    _save_hf(b, pooler=False)
    with pytest.raises(ValueError, match="pooler"):
        read_local_cross_encoder(str(b))


def test_candidate_validation_on_host_arrays():
    from polus_amd.ir.cross import check_candidates
    dev = torch.device("cpu")
    ok = check_candidates(np.array([[0, 4, -1], [2, 2, 3]], np.int64), 2, 5, dev)
    assert ok.dtype == torch.int32 and ok.tolist() == [[0, 4, -1], [2, 2, 3]]
    assert check_candidates(torch.tensor([[1]]), 1, 2, dev).dtype == torch.int32
    for bad, Q in ((np.array([[0, 5]]), 1), (np.array([[-2, 0]]), 1), (np.array([[0.0, 1.0]]), 1), (np.array([0, 1]), 2),
                   (np.array([[0, 1]]), 2), (np.zeros((1, 0), np.int32), 1)):
        with pytest.raises(ValueError):
            check_candidates(bad, Q, 5, dev)


def test_index_and_trainer_refuse_bad_settings_before_touching_a_device():
    from polus_amd.ir.cross import CrossEncoderIndex

    class Cfg:
        max_position_embeddings, vocab_size = 128, 1000

    class Model:
        config = Cfg()
    for kw in (dict(strip=(9, 0)), dict(max_query_tokens=30, max_length=32), dict(max_length=256), dict(cls_token_id=1000),
               dict(tokens_per_batch=0), dict(doc_tokens=0)):
        with pytest.raises(ValueError):
            CrossEncoderIndex(Model(), **dict(dict(max_length=128), **kw))
    idx = CrossEncoderIndex(Model(), max_length=128)
    assert len(idx) == 0 and idx.nbytes == 0
    with pytest.raises(ValueError, match="empty"):
        idx.score({"input_ids": np.zeros((1, 4), np.int32)}, np.array([[0]]))


def test_reexports():
    import polus.ir.cross as a
    import polus.ir.models as m
    import polus.ir.training as t
    import polus.checkpoint as c
    assert a.CrossEncoderIndex and a.RerankValidationCallback and a.plan_buckets
    assert m.CrossEncoder and m.cross_encoder and t.CrossEncoderTrainer and t.PointwiseBCELoss
    assert c.load_cross_encoder_from_local
