"""tests/w4a8_ref.py: the quantiser's edge blocks; test_gpu_w4a8's bar."""
import numpy as np
import pytest

from oracle.moe_oracle import bf16_round
from tests.mxfp4_ref import dequant as dequant_w
from tests.w4a8_ref import dequant, quant_mx32

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("k", [-20, 0, 9])
def test_quantiser_rule_on_edge_blocks(k):
    """Blocks: zero; amax 446, 448, 450 times 2^k (448 * 2^k / 448 is a power
    of two: frexp exponent k + 1); a denormal-sized amax (clamped at -126)."""
    a = np.zeros((1, 5 * 32), dtype=np.float32)
    a[0, 32 + 3], a[0, 64 + 31], a[0, 96] = 446.0, -448.0, 450.0
    a[0, 32:128] *= np.float32(2.0) ** k
    a[0, 33], a[0, 65], a[0, 97] = np.float32(2.0) ** k * np.array([17, 19, 3])
    a[0, 128 + 7] = np.float32(2.0) ** -130
    assert np.array_equal(bf16_round(a), a)
    q, byte = quant_mx32(a)
    assert list(byte[0]) == [127, 127 + k, 128 + k, 128 + k, 1]
    assert not q[0, :32].any()
    assert (q[0, 35], q[0, 95], q[0, 96]) == (448.0, -224.0, 224.0)
    assert (q[0, 33], q[0, 65], q[0, 97]) == (16.0, 10.0, 1.5)  # 17, 9.5: ties
    assert q[0, 135] == 2.0 ** -4
    v = torch.from_numpy(a * np.repeat(np.exp2(127.0 - byte), 32, axis=1)
                         .astype(np.float32))
    assert np.array_equal(v.to(torch.float8_e4m3fn).float().numpy(), q)


@pytest.mark.parametrize("H,P", [(256, 384), (384, 128)])
def test_bar_holds_one_bf16_ulp_of_the_intermediate(H, P):
    """One bf16 ulp on 1e-3 of the intermediate's elements stays inside
    _assert_mx_values' cap at test_gpu_w4a8's shapes and kind of inputs."""
    from tests.test_gpu_parity import _assert_mx_values
    rng = np.random.RandomState(9)
    y = bf16_round(rng.randn(256, P) * np.exp2(np.arange(P) // 32 % 5 - 2))
    flip = rng.rand(*y.shape) < 1e-3
    y1 = np.where(flip, (y.view(np.uint32) + np.uint32(0x10000)).view(
        np.float32), y)
    w_dn = dequant_w(rng.randint(0, 256, (1, 1, H, P // 2)).astype(np.uint8),
                     rng.randint(121, 131, (1, H * P // 32)).astype(np.uint8))
    z, z1 = ((dequant(v) @ w_dn[0, 0].astype(np.float64).T).astype(np.float32)
             for v in (y, y1))
    assert flip.any() and not np.array_equal(z, z1)
    _assert_mx_values(torch.from_numpy(bf16_round(z1)), z)
