"""tests/aquant_ref.py on the CPU: the group128 quantiser's properties, and
that the reference with quantisation off is tests/bscale_ref.py's."""
import numpy as np
import pytest

from oracle.moe_oracle import OracleConfig, _e4m3_pos_grid, bf16_round
from tests.aquant_ref import aquant_moe_forward, dequant, quant_g128
from tests.bscale_ref import bscale_moe_forward, split_record, w_eff

torch = pytest.importorskip("torch")


def rows(n=7, K=384, seed=3):
    rng = np.random.RandomState(seed)
    a = bf16_round(rng.randn(n, K) * np.exp2(rng.randint(-20, 8, (n, 1))))
    a[2, 128:256] = 0.0
    return a


def test_quantiser_properties():
    a = rows()
    q, s = quant_g128(a)
    assert np.isin(np.abs(q), _e4m3_pos_grid()).all()  # on the e4m3 grid
    g, qg = a.reshape(7, 3, 128), q.reshape(7, 3, 128)
    top = np.abs(g).argmax(axis=2)
    at_top = np.take_along_axis(qg, top[:, :, None], axis=2)[:, :, 0]
    zero = np.abs(g).max(axis=2) == 0
    assert zero[2, 1] and zero.sum() == 1
    assert (np.abs(at_top[~zero]) == 448.0).all()  # the amax element
    assert np.array_equal(np.sign(at_top), np.sign(
        np.take_along_axis(g, top[:, :, None], axis=2)[:, :, 0]))
    assert (qg[zero] == 0).all() and (s[zero] == 1.0).all()
    # bit-equal to torch's e4m3 conversion of v / s
    v = torch.from_numpy((g / s[:, :, None]).astype(np.float32))
    assert np.array_equal(v.to(torch.float8_e4m3fn).float().numpy(), qg)


CFG = OracleConfig(num_experts=4, expert_top_k=2, capacity_factor=2,
                   drop_tokens=1, hidden_act=2, element="bf16")


def draw(S=64, H=256, P=128, seed=5):
    rng = np.random.RandomState(seed)
    x = bf16_round(rng.randn(S, H))
    gw = bf16_round(rng.randn(H * 4))
    ew = torch.from_numpy(rng.randn(4, 3, P, H).astype(np.float32)).to(
        torch.float8_e4m3fn).float().numpy()
    sc = np.exp2(rng.randint(-2, 3, (4, 3 * (P // 128) * (H // 128)))).astype(
        np.float32)
    return x, gw, ew, sc


def test_quantisation_off_is_bscale_ref():
    x, gw, ew, sc = draw()
    off = aquant_moe_forward(x, gw, ew, CFG, sc, "block", quant=False)
    assert np.array_equal(off["moe_out"],
                          bscale_moe_forward(x, gw, ew, CFG, sc)["moe_out"])
    on = aquant_moe_forward(x, gw, ew, CFG, sc, "block")
    assert not np.array_equal(on["moe_out"], off["moe_out"])


@pytest.mark.parametrize("H,P", [(384, 256), (256, 384)])
def test_bar_holds_one_bf16_ulp_of_the_intermediate(H, P):
    """One bf16 ulp on 1e-3 of the intermediate's elements stays inside
    _assert_mx_values' cap at the shapes of test_gpu_aquant."""
    from tests.test_gpu_parity import _assert_mx_values

    x, _, ew, sc = draw(S=256, H=H, P=P)
    rng = np.random.RandomState(9)
    y = bf16_round(rng.randn(256, P))  # stands for the rounded intermediate
    flip = rng.rand(*y.shape) < 1e-3
    y1 = np.where(flip, (y.view(np.uint32) + np.uint32(0x10000)).view(
        np.float32), y)
    w_dn = w_eff(ew[0][1].reshape(H, P), split_record(sc[0], P, H, True)[1])
    z, z1 = ((dequant(v) @ w_dn.T).astype(np.float32) for v in (y, y1))
    assert flip.any() and not np.array_equal(z, z1)
    _assert_mx_values(torch.from_numpy(bf16_round(z1)), z)
