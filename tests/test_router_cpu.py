"""Router variants without a GPU: the CPU reference (tests/router_ref.py),
the config contract, the schema and the C-ABI struct."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle.moe_oracle import OracleConfig, moe_forward as oracle_forward
from tests.conftest import REPO_ROOT
from tests.router_ref import (ROUTER_DEFAULTS, router_gate_forward,
                              router_moe_forward)

BASE = {
    "capacity_factor": 1, "drop_tokens": 1, "expert_top_k": 2,
    "global_batch": 256, "is_training": 0, "hidden_act": 0,
    "hidden_size": 128, "intermediate_size": 256, "mini_batch": 1,
    "moe_frequency": 1, "num_experts": 8, "num_layers": 1,
    "sequence_len": 128, "torch_dtype": 2, "vocab_size": 32000,
}


def _cfg_file(tmp_path, **kw):
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(dict(BASE, **kw)))
    return str(p)


# --- the reference

@pytest.mark.parametrize("element, k", [("bf16", 2), ("fp32", 2), ("bf16", 1),
                                        ("fp16", 3)])
def test_default_router_is_the_oracle(element, k):
    """Every key at its default (absent or written out): the reference IS
    oracle.moe_forward, bit for bit."""
    S, H, P, E = 128, 64, 128, 8
    g = torch.Generator().manual_seed(47)
    x = torch.randn(S, H, generator=g).numpy()
    gw = torch.randn(H, E, generator=g).numpy().reshape(-1)
    ew = torch.randn(E, 2, P, H, generator=g).numpy()
    cfg = OracleConfig(num_experts=E, expert_top_k=k, capacity_factor=1,
                       drop_tokens=1, hidden_act=0, element=element)
    want = oracle_forward(x, gw, ew, cfg)
    for router in (None, dict(ROUTER_DEFAULTS)):
        got = router_moe_forward(x, gw, ew, cfg, router)
        for key in ("gate_out", "moe_out", "topk_idx", "eC", "mCw", "kept"):
            assert np.array_equal(got[key], want[key]), key
        assert np.array_equal(got["D"], want["mCw"])  # norm 1, factor 1
        assert np.isinf(got["margin_grp"]).all()


def _one_token(logit_row, E=8):
    """x = [1], gate_w = the logits: one token whose logits are given."""
    x = np.ones((1, 1), dtype=np.float32)
    gate_w = np.asarray(logit_row, dtype=np.float32).reshape(E, 1)
    return x, gate_w


def test_group_limit_excludes_the_globally_best_expert():
    """E = 8, G = 4 (groups {0,1} {2,3} {4,5} {6,7}), TG = 2, k = 2, sigmoid.
    Expert 0 has the best score of all, but under group_score 1 (sum of top
    2) its group {0, 1} = 2.0 - 3.0 loses to {2, 3} and {4, 5}; under
    group_score 0 (max) it wins."""
    cfg = OracleConfig(num_experts=8, expert_top_k=2, element="fp32")
    x, gw = _one_token([2.0, -3.0, 1.5, 1.4, 1.0, 0.9, -1.0, -1.0])
    r = dict(scoring_func=1, n_group=4, topk_group=2)
    top2 = router_gate_forward(x, gw, cfg, dict(r, group_score=1))
    assert top2["topk_idx"].tolist() == [[2, 3]]
    s = 1.0 / (1.0 + np.exp(-np.array([1.5, 1.4])))
    assert np.allclose(top2["mCw"], s.sum(), rtol=1e-6)
    assert np.allclose(top2["D"], s.sum(), rtol=1e-6)  # norm 1, factor 1
    # kept {2,3} and {4,5}; the best dropped group is {0,1}
    sig = lambda v: 1.0 / (1.0 + np.exp(-np.asarray(v, dtype=np.float64)))
    want_gap = sig([1.0, 0.9]).sum() - sig([2.0, -3.0]).sum()
    assert np.allclose(top2["margin_grp"], want_gap, atol=1e-6)
    mx = router_gate_forward(x, gw, cfg, dict(r, group_score=0))
    assert mx["topk_idx"].tolist() == [[0, 2]]
    # without the limit: the two best of all
    free = router_gate_forward(x, gw, cfg, dict(scoring_func=1))
    assert free["topk_idx"].tolist() == [[0, 2]]
    assert np.allclose(free["margin_sel"], sig(1.5) - sig(1.4), atol=1e-6)


def test_bias_changes_selection_but_not_weights():
    cfg = OracleConfig(num_experts=8, expert_top_k=2, element="fp32")
    logits = [2.0, -3.0, 1.5, 1.4, 1.0, 0.9, -1.0, -1.0]
    x, gw = _one_token(logits)
    bias = np.zeros(8, dtype=np.float32)
    bias[7] = 1.0  # sigmoid(-1) + 1 = 1.27 beats sigmoid(2) = 0.88
    r = dict(scoring_func=1, norm_topk_prob=0, routed_scaling_factor=2.5)
    plain = router_gate_forward(x, gw, cfg, r)
    got = router_gate_forward(x, gw, cfg, r, bias)
    assert plain["topk_idx"].tolist() == [[0, 2]]
    assert got["topk_idx"].tolist() == [[7, 0]]
    # gate_out carries s, not c: identical with and without the bias
    assert np.array_equal(got["gate_out"], plain["gate_out"])
    s = 1.0 / (1.0 + np.exp(-np.asarray(logits)))
    assert np.allclose(got["gate_out"][0, :8], s, rtol=1e-6)
    assert np.allclose(got["mCw"], s[7] + s[0], rtol=1e-6)  # raw scores
    assert np.array_equal(got["D"], np.float32([1.0]) / np.float32(2.5))
    # ... so the applied weight of expert 7 is s[7] * 2.5, not (s[7] + 1) * 2.5
    assert np.allclose(got["gate_out"][0, 7] / got["D"], s[7] * 2.5, rtol=1e-6)


def test_tie_rule_first_index_for_experts_and_groups():
    cfg = OracleConfig(num_experts=8, expert_top_k=2, element="fp32")
    x, gw = _one_token([0.0] * 8)
    got = router_gate_forward(x, gw, cfg, dict(
        scoring_func=1, n_group=4, topk_group=2, group_score=1))
    assert got["topk_idx"].tolist() == [[0, 1]]  # groups 0, 1; experts 0, 1
    assert got["margin_sel"][0] == 0 and got["margin_grp"][0] == 0


def test_scaling_factor_doubles_the_output_exactly():
    S, H, P, E = 128, 64, 128, 8
    g = torch.Generator().manual_seed(47)
    x = torch.randn(S, H, generator=g).numpy()
    gw = (torch.randn(H, E, generator=g) / H ** 0.5).numpy().reshape(-1)
    ew = (torch.randn(E, 2, P, H, generator=g) / 16).numpy()
    for element in ("bf16", "fp32"):
        cfg = OracleConfig(num_experts=E, expert_top_k=2, capacity_factor=2,
                           element=element)
        one = router_moe_forward(x, gw, ew, cfg)
        two = router_moe_forward(x, gw, ew, cfg,
                                 dict(routed_scaling_factor=2.0))
        assert np.abs(one["moe_out"]).max() > 0.1
        assert np.array_equal(two["moe_out"], 2 * one["moe_out"])
        assert np.array_equal(two["D"], one["D"] / 2)


# --- config contract

def test_load_config_router_keys(tmp_path):
    from flashmoe_amd.config import (ROUTER_DEFAULTS as CFG_DEFAULTS,
                                     load_config, router_is_default, router_of)

    assert CFG_DEFAULTS == ROUTER_DEFAULTS
    assert router_of(load_config()) == ROUTER_DEFAULTS  # the committed config
    assert router_is_default(load_config(_cfg_file(tmp_path)))
    v3 = dict(num_experts=256, expert_top_k=8, scoring_func=1, n_group=8,
              topk_group=4, group_score=1, norm_topk_prob=1,
              routed_scaling_factor=2.5)
    cfg = load_config(_cfg_file(tmp_path, **v3))
    assert not router_is_default(cfg)
    assert router_of(cfg) == {k: v3[k] for k in ROUTER_DEFAULTS}
    # explicit defaults are the default router
    assert router_is_default(load_config(_cfg_file(tmp_path,
                                                   **ROUTER_DEFAULTS)))


@pytest.mark.parametrize("kw, key", [
    (dict(n_group=3), "n_group"),                        # 8 % 3
    (dict(n_group=0), "n_group"),
    (dict(num_experts=64, n_group=32, topk_group=32), "n_group"),  # > 16
    (dict(n_group=4, topk_group=5), "topk_group"),
    (dict(n_group=4, topk_group=0), "topk_group"),
    (dict(n_group=8, topk_group=1), "expert_top_k"),     # 2 > 1 * 8 / 8
    (dict(n_group=8, topk_group=8, group_score=1), "group_score"),
    (dict(routed_scaling_factor=0), "routed_scaling_factor"),
    (dict(routed_scaling_factor=-1.0), "routed_scaling_factor"),
    (dict(routed_scaling_factor=float("inf")), "routed_scaling_factor"),
    (dict(routed_scaling_factor=float("nan")), "routed_scaling_factor"),
    (dict(expert_top_k=1, norm_topk_prob=0), "norm_topk_prob"),
    (dict(expert_top_k=1, routed_scaling_factor=2.0), "routed_scaling_factor"),
    (dict(is_training=1, scoring_func=1), "scoring_func"),
    (dict(is_training=1, routed_scaling_factor=2.0), "routed_scaling_factor"),
    (dict(num_experts=512, scoring_func=1), "scoring_func"),
    (dict(num_experts=512, n_group=8, topk_group=4), "n_group"),
    (dict(scoring_func=2), "scoring_func"),
    (dict(norm_topk_prob=2), "norm_topk_prob"),
    (dict(group_score=True), "group_score"),
])
def test_load_config_refuses(tmp_path, kw, key):
    from flashmoe_amd.config import load_config

    with pytest.raises(ValueError, match=key):
        load_config(_cfg_file(tmp_path, **kw))


def test_load_config_accepts_what_fm_set_router_accepts(tmp_path):
    from flashmoe_amd.config import load_config

    # norm / factor alone work at every E
    load_config(_cfg_file(tmp_path, num_experts=512, norm_topk_prob=0,
                          routed_scaling_factor=16.0))
    # top-1 with sigmoid scoring, normalised, factor 1: unscaled as ever
    load_config(_cfg_file(tmp_path, expert_top_k=1, scoring_func=1))
    # training with explicit defaults
    load_config(_cfg_file(tmp_path, is_training=1, **ROUTER_DEFAULTS))


def test_schema_carries_the_router_keys():
    with open(os.path.join(REPO_ROOT, "csrc",
                           "flashmoe_config.schema.json")) as f:
        schema = json.load(f)
    props = schema["properties"]
    for key, default in ROUTER_DEFAULTS.items():
        assert key in props and key not in schema["required"]
        assert props[key]["default"] == default
    for key in ("scoring_func", "norm_topk_prob", "group_score"):
        assert props[key]["enum"] == [0, 1]
    assert props["n_group"]["minimum"] == 1 and props["n_group"]["maximum"] == 16
    assert props["routed_scaling_factor"]["exclusiveMinimum"] == 0
    with open(os.path.join(REPO_ROOT, "csrc", "flashmoe_config.json")) as f:
        assert not set(ROUTER_DEFAULTS) & set(json.load(f))  # absent = default


# --- C-ABI

def test_router_struct_and_header():
    import flashmoe_amd._ext as _ext

    fields = _ext.FMRouterConfig._fields_
    assert [f[0] for f in fields] == [
        "scoring_func", "norm_topk_prob", "n_group", "topk_group",
        "group_score", "routed_scaling_factor", "score_bias"]
    assert all(f[1] is ctypes.c_int32 for f in fields[:5])
    assert fields[5][1] is ctypes.c_float and fields[6][1] is ctypes.c_void_p
    assert ctypes.sizeof(_ext.FMRouterConfig) == 32
    assert _ext.FMRouterConfig.score_bias.offset == 24
    d = _ext.router_defaults()
    assert (d.scoring_func, d.norm_topk_prob, d.n_group, d.topk_group,
            d.group_score, d.routed_scaling_factor, d.score_bias) == \
        (0, 1, 1, 1, 0, 1.0, None)
    # fm_config did not grow
    assert ctypes.sizeof(_ext.FMConfig) == 48
    with open(os.path.join(REPO_ROOT, "include", "flashmoe_abi.h")) as f:
        hdr = f.read()
    assert re.search(
        r"int\s+fm_set_router\s*\(\s*const\s+fm_router_config\s*\*\s*\w+\s*\)\s*;",
        hdr)
    assert re.search(
        r"int\s+fm_get_router\s*\(\s*fm_router_config\s*\*\s*\w+\s*\)\s*;", hdr)
    body = re.search(
        r"typedef struct fm_router_config \{(.*?)\} fm_router_config;", hdr,
        re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*;", body)
    assert names == [f[0] for f in fields]


def test_library_exports_the_router_entry_points():
    from tests.test_abi import _built

    lib = ctypes.CDLL(_built())
    assert lib.fm_set_router is not None and lib.fm_get_router is not None
    import flashmoe_amd._ext as _ext

    bound = _ext.load()
    # before fm_initialize both refuse with a state error, touching no GPU
    assert bound.fm_set_router(None) == -2
    out = _ext.FMRouterConfig()
    assert bound.fm_get_router(ctypes.byref(out)) == -2
