"""Gated experts (hidden_act 2 SwiGLU / 3 GeGLU): the CPU reference in
tests/gated_ref.py, the config contract and the schema."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle.moe_oracle import OracleConfig
from tests.conftest import REPO_ROOT
from tests.gated_ref import gated_expert_ffn, gated_moe_forward


def _cfg_file(tmp_path, **kw):
    cfg = {
        "capacity_factor": 1, "drop_tokens": 1, "expert_top_k": 2,
        "global_batch": 256, "is_training": 0, "hidden_act": 0,
        "hidden_size": 128, "intermediate_size": 256, "mini_batch": 1,
        "moe_frequency": 1, "num_experts": 8, "num_layers": 1,
        "sequence_len": 128, "torch_dtype": 2, "vocab_size": 32000,
    }
    cfg.update(kw)
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(cfg))
    return str(p)


@pytest.mark.parametrize("act", [2, 3])
def test_gated_ffn_matches_torch(act):
    g = torch.Generator().manual_seed(47)
    n, H, P = 48, 64, 96
    x = torch.randn(n, H, generator=g, dtype=torch.float64)
    Wu = torch.randn(P, H, generator=g, dtype=torch.float64)
    Wd = torch.randn(H, P, generator=g, dtype=torch.float64)
    Wg = torch.randn(P, H, generator=g, dtype=torch.float64)
    F = torch.nn.functional
    gate = F.silu(x @ Wg.T) if act == 2 else F.gelu(x @ Wg.T, approximate="none")
    want = ((gate * (x @ Wu.T)) @ Wd.T).numpy()
    got = gated_expert_ffn(
        x.numpy().astype(np.float32), Wu.numpy().astype(np.float32),
        Wd.numpy().astype(np.float32).reshape(-1),
        Wg.numpy().astype(np.float32), act, "fp32")
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-5 * scale


def test_zero_up_projection_gives_zero_output():
    g = torch.Generator().manual_seed(47)
    S, H, P, E = 128, 64, 128, 4
    x = torch.randn(S, H, generator=g).numpy()
    gw = torch.randn(H, E, generator=g).numpy().reshape(-1)
    ew = torch.randn(E, 3, P, H, generator=g).numpy()
    ew[:, 0] = 0.0  # Wup rows all zero -> u == 0 -> h == 0
    cfg = OracleConfig(num_experts=E, expert_top_k=1, capacity_factor=1,
                       drop_tokens=1, hidden_act=2, element="fp32")
    ref = gated_moe_forward(x, gw, ew, cfg)
    assert ref["moe_out"].shape == (S, H)
    assert not ref["moe_out"].any()


def test_load_config_gated(tmp_path):
    from flashmoe_amd.config import load_config

    assert load_config(_cfg_file(tmp_path, hidden_act=2))["hidden_act"] == 2
    assert load_config(_cfg_file(tmp_path, hidden_act=3))["hidden_act"] == 3
    with pytest.raises(ValueError, match="hidden_act"):
        load_config(_cfg_file(tmp_path, hidden_act=4))
    for act in (2, 3):
        with pytest.raises(ValueError) as ei:
            load_config(_cfg_file(tmp_path, hidden_act=act, torch_dtype=5))
        assert "hidden_act" in str(ei.value) and "torch_dtype" in str(ei.value)
    # the non-gated MX config still loads
    assert load_config(_cfg_file(tmp_path, torch_dtype=5))["torch_dtype"] == 5


def test_expert_mats_and_is_gated():
    from flashmoe_amd.config import expert_mats, is_gated

    assert [expert_mats(a) for a in range(4)] == [2, 2, 3, 3]
    assert [is_gated(a) for a in range(4)] == [False, False, True, True]


def test_schema_enum_has_gated_values():
    with open(os.path.join(REPO_ROOT, "csrc",
                           "flashmoe_config.schema.json")) as f:
        schema = json.load(f)
    enum = schema["properties"]["hidden_act"]["enum"]
    assert enum == [0, 1, 2, 3]
