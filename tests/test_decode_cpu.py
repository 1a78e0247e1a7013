"""Decode-sized configs (S = sequence_len * mini_batch in 1..127) on the CPU:
what load_config and the schema accept and refuse."""
import json
import os

import pytest

from flashmoe_amd.config import load_config, num_tokens
from tests.conftest import REPO_ROOT

BASE = {
    "capacity_factor": 1, "drop_tokens": 1, "expert_top_k": 2,
    "global_batch": 256, "is_training": 0, "hidden_act": 0,
    "hidden_size": 128, "intermediate_size": 256, "mini_batch": 1,
    "moe_frequency": 1, "num_experts": 8, "num_layers": 1,
    "sequence_len": 128, "torch_dtype": 2, "vocab_size": 32000,
}


def write_cfg(tmp_path, **kw):
    cfg = dict(BASE, **kw)
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(cfg))
    return str(p)


@pytest.mark.parametrize("S", [1, 7, 127])
@pytest.mark.parametrize("as_batch", [True, False])
def test_decode_products_are_accepted(tmp_path, S, as_batch):
    kw = dict(sequence_len=1, mini_batch=S) if as_batch else \
        dict(sequence_len=S, mini_batch=1)
    cfg = load_config(write_cfg(tmp_path, **kw))
    assert num_tokens(cfg) == S


@pytest.mark.parametrize("sl,mb", [(128, 1), (64, 2), (128, 3), (1, 256)])
def test_multiples_of_128_are_still_accepted(tmp_path, sl, mb):
    cfg = load_config(write_cfg(tmp_path, sequence_len=sl, mini_batch=mb))
    assert num_tokens(cfg) == sl * mb


@pytest.mark.parametrize("sl,mb", [(0, 1), (1, 0), (129, 1), (1, 129),
                                   (200, 1), (100, 2), (8, 25)])
def test_other_products_are_refused(tmp_path, sl, mb):
    assert sl * mb in (0, 129, 200)
    with pytest.raises(ValueError, match="sequence_len \\* mini_batch"):
        load_config(write_cfg(tmp_path, sequence_len=sl, mini_batch=mb))


def test_decode_refuses_mx(tmp_path):
    with pytest.raises(ValueError, match="torch_dtype=5"):
        load_config(write_cfg(tmp_path, sequence_len=1, mini_batch=64,
                              torch_dtype=5))
    # the same config at 128 tokens is fine
    load_config(write_cfg(tmp_path, sequence_len=1, mini_batch=128,
                          torch_dtype=5))


def test_decode_refuses_training(tmp_path):
    with pytest.raises(ValueError, match="is_training=1"):
        load_config(write_cfg(tmp_path, sequence_len=1, mini_batch=64,
                              is_training=1))
    load_config(write_cfg(tmp_path, sequence_len=128, is_training=1))


def test_schema_has_no_multiple_of_on_sequence_len():
    with open(os.path.join(REPO_ROOT, "csrc",
                           "flashmoe_config.schema.json")) as f:
        schema = json.load(f)
    prop = schema["properties"]["sequence_len"]
    assert "multipleOf" not in prop
    assert prop["type"] == "integer" and prop["minimum"] == 1
