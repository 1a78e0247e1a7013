"""Per-output-channel weight scales (fm_set_weight_scales): the CPU reference
in tests/wscale_ref.py, pack_weight_scales, the header and the Python
contract that needs no GPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle.moe_oracle import OracleConfig, moe_forward as oracle_forward
from tests.gated_ref import gated_moe_forward
from tests.shared_ref import shared_moe_forward
from tests.test_abi import header_symbols
from tests.wscale_ref import wscale_moe_forward

S, H, P, E = 128, 128, 256, 8


def draw(mats, n_exp=E, seed=47, fp8=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, H, generator=g).to(torch.bfloat16).float().numpy()
    gw = torch.randn(H, E, generator=g).to(torch.bfloat16).float().numpy()
    ew = torch.randn(n_exp, mats, P, H, generator=g)
    if fp8:
        ew = ew.to(torch.float8_e4m3fn)
    return x, gw.reshape(-1), ew.float().numpy()


def ocfg(**kw):
    kw.setdefault("element", "bf16")
    return OracleConfig(num_experts=E, expert_top_k=2, capacity_factor=1,
                        drop_tokens=1, **kw)


def ones(n_exp, gated):
    return np.ones((n_exp, P + H + (P if gated else 0)), dtype=np.float32)


# --- all-ones scales: exactly the existing references

def test_ones_equal_oracle_relu():
    x, gw, ew = draw(2)
    cfg = ocfg(hidden_act=0)
    want = oracle_forward(x, gw, ew, cfg)
    got = wscale_moe_forward(x, gw, ew, cfg, ones(E, False))
    assert np.array_equal(got["moe_out"], want["moe_out"])
    assert np.array_equal(got["gate_out"], want["gate_out"])


def test_ones_equal_oracle_gelu_biases():
    x, gw, ew = draw(2)
    g = torch.Generator().manual_seed(321)
    b_up = torch.randn(E, P, generator=g).to(torch.bfloat16).float().numpy()
    b_dn = torch.randn(E, H, generator=g).to(torch.bfloat16).float().numpy()
    cfg = ocfg(hidden_act=1)
    want = oracle_forward(x, gw, ew, cfg, b_up=b_up, b_dn=b_dn)
    got = wscale_moe_forward(x, gw, ew, cfg, ones(E, False), b_up=b_up,
                             b_dn=b_dn)
    assert np.array_equal(got["moe_out"], want["moe_out"])


def test_ones_equal_gated_ref_swiglu():
    x, gw, ew = draw(3)
    cfg = ocfg(hidden_act=2)
    want = gated_moe_forward(x, gw, ew, cfg)
    got = wscale_moe_forward(x, gw, ew, cfg, ones(E, True))
    assert np.array_equal(got["moe_out"], want["moe_out"])


def test_ones_equal_shared_ref_swiglu_one_shared():
    x, gw, ew = draw(3, n_exp=E + 1)
    cfg = ocfg(hidden_act=2)
    want = shared_moe_forward(x, gw, ew, cfg, 1)
    got = wscale_moe_forward(x, gw, ew, cfg, ones(E + 1, True), n_shared=1)
    assert np.array_equal(got["moe_out"], want["moe_out"])


def test_ones_equal_oracle_mx_relu():
    x, gw, ew = draw(2)
    cfg = ocfg(hidden_act=0, mx_fp8=True)
    want = oracle_forward(x, gw, ew, cfg)
    got = wscale_moe_forward(x, gw, ew, cfg, ones(E, False))
    assert np.array_equal(got["moe_out"], want["moe_out"])


# --- the record layout: against scaled WEIGHTS, where nothing rounds (fp32)

@pytest.mark.parametrize("act", [1, 2])
def test_scales_equal_scaled_weights_in_fp32(act):
    """In fp32 nothing is rounded to an element type, so scaling the matmul
    result per column and scaling the weight rows agree to fp32 rounding.
    Pins [s_up | s_dn | s_glu] and the [H, P] use of the down buffer."""
    gated = act >= 2
    x, gw, ew = draw(3 if gated else 2, fp8=False)
    g = torch.Generator().manual_seed(48)
    sc = torch.exp2(3.0 * torch.rand(E, P + H + (P if gated else 0),
                                     generator=g) - 2.0).numpy()
    cfg = ocfg(hidden_act=act, element="fp32")
    got = wscale_moe_forward(x, gw, ew, cfg, sc)["moe_out"]
    weff = ew.copy()
    weff[:, 0] *= sc[:, :P, None]
    weff[:, 1] = (ew[:, 1].reshape(E, H, P) *
                  sc[:, P:P + H, None]).reshape(E, P, H)
    if gated:
        weff[:, 2] *= sc[:, P + H:, None]
        want = gated_moe_forward(x, gw, weff, cfg)["moe_out"]
    else:
        want = oracle_forward(x, gw, weff, cfg)["moe_out"]
    unscaled = wscale_moe_forward(x, gw, ew, cfg, ones(E, gated))["moe_out"]
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-4 * scale
    assert np.abs(unscaled - want).max() > 1e-1 * scale  # the scales matter


# --- pack_weight_scales

def test_pack_layout():
    from flashmoe_amd import moe

    up = torch.arange(6.0).reshape(2, 3)
    dn = torch.arange(4.0).reshape(2, 2) + 10
    glu = torch.arange(6.0).reshape(2, 3) + 20
    got = moe.pack_weight_scales(up, dn)
    assert got.dtype == torch.float32 and got.is_contiguous()
    assert got.tolist() == [[0, 1, 2, 10, 11], [3, 4, 5, 12, 13]]
    got = moe.pack_weight_scales(up, dn, glu)
    assert got.tolist() == [[0, 1, 2, 10, 11, 20, 21, 22],
                            [3, 4, 5, 12, 13, 23, 24, 25]]


def test_pack_broadcasting():
    from flashmoe_amd import moe

    up = torch.arange(6.0).reshape(2, 3)
    dn = torch.arange(4.0).reshape(2, 2) + 10
    # per-tensor: one value per (expert, matrix), or one for all experts
    got = moe.pack_weight_scales(torch.tensor([7.0, 8.0]), dn, up)
    assert got.tolist() == [[7, 7, 7, 10, 11, 0, 1, 2],
                            [8, 8, 8, 12, 13, 3, 4, 5]]
    got = moe.pack_weight_scales(up, dn, torch.tensor(0.5, dtype=torch.float64))
    assert got.dtype == torch.float32
    assert got.tolist() == [[0, 1, 2, 10, 11, .5, .5, .5],
                            [3, 4, 5, 12, 13, .5, .5, .5]]
    # size-1 dimensions broadcast, they are never a width or an expert
    # count: [nE, 1] (torch.stack of per-tensor [1] scales) and a lone [1]
    got = moe.pack_weight_scales(torch.tensor([[7.0], [8.0]]), dn, up)
    assert got.tolist() == [[7, 7, 7, 10, 11, 0, 1, 2],
                            [8, 8, 8, 12, 13, 3, 4, 5]]
    got = moe.pack_weight_scales(torch.tensor([9.0]), torch.tensor([[1., 2.]]),
                                 up)
    assert got.tolist() == [[9, 9, 9, 1, 2, 0, 1, 2], [9, 9, 9, 1, 2, 3, 4, 5]]
    with pytest.raises(ValueError, match="infer P"):  # ungated, up [nE, 1]
        moe.pack_weight_scales(torch.ones(4, 1), torch.ones(4, 6))
    with pytest.raises(ValueError, match="infer H"):
        moe.pack_weight_scales(up, torch.tensor(2.0))
    with pytest.raises(ValueError):  # up and glu disagree on P
        moe.pack_weight_scales(up, dn, torch.ones(2, 4))
    with pytest.raises(ValueError):  # expert counts disagree
        moe.pack_weight_scales(up, torch.ones(3, 2))


# --- header and Python contract

def test_header_declares_the_weight_scale_symbols():
    syms = header_symbols()
    assert "fm_set_weight_scales" in syms
    assert "fm_get_weight_scales" in syms


def test_set_before_initialize_raises():
    from flashmoe_amd import moe

    with pytest.raises(RuntimeError, match="initialize"):
        moe.set_weight_scales(torch.ones(E, P + H))
    with pytest.raises(RuntimeError, match="initialize"):
        moe.set_weight_scales(None)
    with pytest.raises(RuntimeError, match="initialize"):
        moe.get_weight_scales()


def test_packages_export_the_api():
    import flashmoe
    import flashmoe_amd

    for name in ("set_weight_scales", "get_weight_scales",
                 "pack_weight_scales"):
        assert getattr(flashmoe, name) is getattr(flashmoe_amd, name)
