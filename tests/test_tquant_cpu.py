"""tests/tquant_ref.py on the CPU: the token quantiser's properties, that
test_gpu_tquant's bar holds one bf16 ulp of the intermediate, and how far the
token reference lies from the group128 and the unquantised ones."""
import numpy as np
import pytest

from oracle.moe_oracle import OracleConfig, _e4m3_pos_grid, bf16_round
from tests.tquant_ref import dequant, quant_row, tquant_moe_forward

torch = pytest.importorskip("torch")


def test_quantiser_properties():
    rng = np.random.RandomState(3)
    a = bf16_round(rng.randn(7, 384) * np.exp2(rng.randint(-20, 8, (7, 1))))
    a[2] = 0.0
    q, s = quant_row(a)
    assert np.isin(np.abs(q), _e4m3_pos_grid()).all() and np.abs(q).max() <= 448
    top = np.abs(a).argmax(axis=1)
    at_top, live = q[np.arange(7), top], np.arange(7) != 2
    assert (np.abs(at_top[live]) == 448.0).all()  # the amax element
    assert np.array_equal(np.sign(at_top), np.sign(a[np.arange(7), top]))
    assert (q[2] == 0).all() and s[2] == 1.0
    v = torch.from_numpy((a / s[:, None]).astype(np.float32))
    assert np.array_equal(v.to(torch.float8_e4m3fn).float().numpy(), q)


CFG = OracleConfig(num_experts=4, expert_top_k=2, capacity_factor=2,
                   drop_tokens=1, hidden_act=2, element="bf16")


def draw(H, P, S=256, seed=5):
    """test_gpu_tquant's kind of inputs: row r of x times 2^((r % 5) - 2),
    per-channel scales exp2(U(-2, 1))."""
    rng = np.random.RandomState(seed)
    x = bf16_round(rng.randn(S, H) * np.exp2(np.arange(S) % 5 - 2)[:, None])
    gw = bf16_round(rng.randn(H * 4))
    ew = torch.from_numpy(rng.randn(4, 3, P, H).astype(np.float32)).to(
        torch.float8_e4m3fn).float().numpy()
    sc = np.exp2(3.0 * rng.rand(4, 2 * P + H) - 2.0).astype(np.float32)
    return x, gw, ew, sc


@pytest.mark.parametrize("H,P", [(384, 256), (256, 384)])
def test_bar_holds_one_bf16_ulp_of_the_intermediate(H, P):
    """One bf16 ulp on 1e-3 of the intermediate's elements stays inside
    _assert_mx_values' cap at the shapes of test_gpu_tquant; and the distances
    between the three references."""
    from tests.test_gpu_parity import _assert_mx_values

    x, gw, ew, sc = draw(H, P)
    rng = np.random.RandomState(9)
    y = bf16_round(rng.randn(256, P) * np.exp2(np.arange(256) % 5 - 2)[:, None])
    flip = rng.rand(*y.shape) < 1e-3
    y1 = np.where(flip, (y.view(np.uint32) + np.uint32(0x10000)).view(
        np.float32), y)
    w_dn = ew[0][1].reshape(H, P).astype(np.float64)
    z, z1 = ((dequant(v) @ w_dn.T).astype(np.float32) * sc[0][P:P + H]
             for v in (y, y1))
    assert flip.any() and not np.array_equal(z, z1)
    _assert_mx_values(torch.from_numpy(bf16_round(z1)), z)
    ref = {m: tquant_moe_forward(x, gw, ew, CFG, sc, mode=m)["moe_out"]
           for m in ("token", "group128", None)}
    rms = lambda a: float(np.sqrt(np.mean(np.square(a, dtype=np.float64))))
    print(f"H {H} P {P}: rms(ref_token) {rms(ref['token']):.4f}, "
          f"rms(ref_token - ref_group128) "
          f"{rms(ref['token'] - ref['group128']):.5f}, "
          f"rms(ref_token - ref_unquantised) {rms(ref['token'] - ref[None]):.5f}")
    assert not np.array_equal(ref["token"], ref["group128"])
