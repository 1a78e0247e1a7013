"""128x128 block scales (fm_set_weight_block_scales): pack_weight_block_scales,
its validation, and the CPU reference in tests/bscale_ref.py. No GPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle.moe_oracle import OracleConfig
from tests.bscale_ref import bscale_moe_forward
from tests.wscale_ref import wscale_moe_forward


def test_pack_layout_against_a_hand_written_record():
    """nE = 2, PB = 2, HB = 3: up / glu are [PB, HB], down is [HB, PB], each
    flattened row-major, records [s_up | s_dn | s_glu]."""
    from flashmoe_amd import moe

    up = torch.arange(12.0).reshape(2, 2, 3)
    dn = torch.arange(12.0).reshape(2, 3, 2) + 100
    glu = torch.arange(12.0).reshape(2, 2, 3) + 200
    got = moe.pack_weight_block_scales(up, dn, glu)
    assert got.dtype == torch.float32 and got.is_contiguous()
    assert got.tolist() == [
        [0, 1, 2, 3, 4, 5, 100, 101, 102, 103, 104, 105,
         200, 201, 202, 203, 204, 205],
        [6, 7, 8, 9, 10, 11, 106, 107, 108, 109, 110, 111,
         206, 207, 208, 209, 210, 211]]
    assert moe.pack_weight_block_scales(up, dn).tolist() == \
        [r[:12] for r in got.tolist()]
    # per-tensor scales: [nE] per expert, 0-dim for all experts
    got = moe.pack_weight_block_scales(torch.tensor([7.0, 8.0]), dn,
                                       torch.tensor(0.5))
    assert got[:, :6].tolist() == [[7.0] * 6, [8.0] * 6]
    assert got[:, 12:].eq(0.5).all() and got[1, 6:12].tolist() == \
        [106, 107, 108, 109, 110, 111]


def test_pack_validation():
    from flashmoe_amd import moe

    up = torch.ones(2, 2, 3)
    with pytest.raises(ValueError, match="disagree"):  # down not transposed
        moe.pack_weight_block_scales(up, torch.ones(2, 2, 3))
    with pytest.raises(ValueError, match="disagree"):  # expert counts
        moe.pack_weight_block_scales(up, torch.ones(3, 3, 2))
    with pytest.raises(ValueError, match="disagree"):
        moe.pack_weight_block_scales(up, torch.ones(3))
    with pytest.raises(ValueError, match="0-dim"):  # a per-channel vector
        moe.pack_weight_block_scales(torch.ones(2, 256), torch.ones(2, 3, 2))
    with pytest.raises(ValueError, match="infer"):
        moe.pack_weight_block_scales(torch.tensor(1.0), torch.tensor(2.0))
    with pytest.raises(RuntimeError, match="initialize"):
        moe.set_weight_block_scales(torch.ones(2, 12))


def test_all_ones_equal_the_per_channel_reference_with_all_ones():
    """Up to float64 / float32 matmul rounding under the bf16 roundings."""
    S, H, P, E = 128, 256, 128, 4
    g = torch.Generator().manual_seed(47)
    x = torch.randn(S, H, generator=g).to(torch.bfloat16).float().numpy()
    gw = torch.randn(H, E, generator=g).to(torch.bfloat16).float().numpy()
    ew = torch.randn(E + 1, 3, P, H, generator=g).to(
        torch.float8_e4m3fn).float().numpy()
    cfg = OracleConfig(num_experts=E, expert_top_k=2, capacity_factor=2,
                       drop_tokens=1, hidden_act=2, element="bf16")
    want = wscale_moe_forward(x, gw.reshape(-1), ew, cfg,
                              np.ones((E + 1, 2 * P + H), np.float32),
                              n_shared=1)["moe_out"]
    got = bscale_moe_forward(x, gw.reshape(-1), ew, cfg,
                             np.ones((E + 1, 3 * 2), np.float32),
                             n_shared=1)["moe_out"]
    # bf16 has 8 bits: a one-ulp flip of a rounded value is 2^-8 relative
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 2.0 ** -7 * scale
    assert np.mean(got == want) > 0.95
