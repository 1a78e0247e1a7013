"""MXFP4 (torch_dtype 6) on the CPU: config, scale packing, reference dequant."""
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from flashmoe_amd import moe
from flashmoe_amd.config import (element_size_of, load_config, torch_dtype_of,
                                 weight_dtype_of)
from tests.conftest import REPO_ROOT
from tests.mxfp4_ref import dequant

BASE = {
    "capacity_factor": 1, "drop_tokens": 1, "expert_top_k": 2,
    "global_batch": 256, "is_training": 0, "hidden_act": 2,
    "hidden_size": 256, "intermediate_size": 384, "mini_batch": 1,
    "moe_frequency": 1, "num_experts": 4, "num_layers": 1,
    "sequence_len": 256, "torch_dtype": 6, "vocab_size": 32000,
}


def write(tmp_path, **kw):
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(dict(BASE, **kw)))
    return str(p)


def test_config_contract(tmp_path):
    assert load_config(write(tmp_path))["torch_dtype"] == 6
    with pytest.raises(ValueError, match="128"):
        load_config(write(tmp_path, hidden_size=192))
    with pytest.raises(ValueError, match="is_training"):
        load_config(write(tmp_path, is_training=1))
    with open(f"{REPO_ROOT}/csrc/flashmoe_config.schema.json") as f:
        assert 6 in json.load(f)["properties"]["torch_dtype"]["enum"]
    assert weight_dtype_of(6) == torch.uint8
    assert torch_dtype_of(6) == torch.bfloat16 and element_size_of(6) == 2


@pytest.mark.parametrize("gated,n_shared", [(False, 0), (True, 0), (True, 1)])
def test_pack_record_order(gated, n_shared):
    nE, P, H = 2 + n_shared, 64, 96
    g = torch.Generator().manual_seed(5)
    up = torch.randint(1, 255, (nE, P, H // 32), generator=g, dtype=torch.uint8)
    dn = torch.randint(1, 255, (nE, H, P // 32), generator=g, dtype=torch.uint8)
    glu = torch.randint(1, 255, (nE, P, H // 32), generator=g,
                        dtype=torch.uint8) if gated else None
    got = moe.pack_weight_mx_scales(up, dn, glu)
    part = P * H // 32
    assert got.dtype == torch.uint8 and got.is_contiguous()
    assert tuple(got.shape) == (nE, (3 if gated else 2) * part)
    e = nE - 1  # the shared expert's record, when there is one, is the last
    assert got[e, 5 * (H // 32) + 2] == up[e, 5, 2]
    assert got[e, part + 7 * (P // 32) + 1] == dn[e, 7, 1]
    if gated:
        assert got[e, 2 * part + 63 * (H // 32)] == glu[e, 63, 0]


def test_dequant_table():
    """16 codes x bytes {1, 127, 254}; 2, 3, 4, 6 at 254 exceed fp32: inf."""
    mags = [0, 0.5, 1, 1.5, 2, 3, 4, 6]
    table = mags + [-m for m in mags]
    # one expert, 2 slots, P = 1, H = 32: byte j = code j (low), 15 - j (high)
    row = np.array([j | ((15 - j) << 4) for j in range(16)], dtype=np.uint8)
    w = np.stack([row, row]).reshape(1, 2, 1, 16)
    for byte in (1, 127, 254):
        got = dequant(w, np.array([[byte, 127]], dtype=np.uint8))
        want = np.array([table[j // 2] if j % 2 == 0 else table[15 - j // 2]
                         for j in range(32)], dtype=np.float64)
        scaled = want * 2.0 ** (byte - 127)
        scaled[np.abs(scaled) >= 2.0 ** 128] *= np.inf
        assert np.array_equal(got[0, 0, 0], scaled)
        assert np.isinf(got[0, 0, 0]).sum() == (16 if byte == 254 else 0)
        assert np.array_equal(got[0, 1, 0], want)
    assert np.signbit(dequant(w, np.full((1, 2), 127, np.uint8))[0, 0, 0, 16])
