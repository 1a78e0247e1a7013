"""CPU reference for fm_set_activation_quant(3), "mxfp8" (DESIGN.md par.5q):
the project's MX rule (oracle.mx_quant_rows) per block of 32 along K,

    amax = max|v|;  e = 0 for a zero block, else frexp(amax / 448)'s exponent,
    clamped to -126..127;  byte = 127 + e;  q = e4m3_rne(v * 2^-e)

Both expert GEMMs see q * 2^(byte - 127) in float64 in the place of the
activation, over tests/mxfp4_ref.dequant's weights with unit scale records."""
import numpy as np

from oracle.moe_oracle import e4m3_round
from tests import aquant_ref, wscale_ref


def quant_mx32(a):
    """(q [n, K] fp32 on the e4m3 grid, byte [n, K / 32] uint8) of rows a."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    n, K = a.shape
    blocks = a.reshape(n, K // 32, 32).astype(np.float64)
    amax = np.abs(blocks).max(axis=2)
    e = np.zeros(amax.shape, dtype=np.int64)
    e[amax > 0] = np.frexp(amax[amax > 0] / 448.0)[1]
    e = np.clip(e, -126, 127)
    q = e4m3_round(blocks * np.exp2(-e.astype(np.float64))[:, :, None])
    return q.reshape(n, K), (127 + e).astype(np.uint8)


def dequant(a, quant=True):
    q, byte = quant_mx32(a)
    return q.astype(np.float64) * np.repeat(
        np.exp2(byte.astype(np.float64) - 127.0), 32, axis=1)


def expert_ffn(*args, **kw):
    # aquant_ref's per-channel expert FFN with this quantiser
    saved, aquant_ref.dequant = aquant_ref.dequant, dequant
    try:
        return aquant_ref.make_expert_ffn("channel")(*args, **kw)
    finally:
        aquant_ref.dequant = saved


def w4a8_moe_forward(x, gate_w_buffer, w_eff, cfg, n_shared=0, b_up=None,
                     b_dn=None):
    """wscale_moe_forward over w_eff [nE, mats, P, H], unit scale records."""
    nE, mats, P, H = w_eff.shape
    ones = np.ones((nE, P + H + (P if mats == 3 else 0)), dtype=np.float32)
    saved, wscale_ref.wscale_expert_ffn = wscale_ref.wscale_expert_ffn, expert_ffn
    try:
        return wscale_ref.wscale_moe_forward(x, gate_w_buffer, w_eff, cfg, ones,
                                             n_shared, b_up, b_dn)
    finally:
        wscale_ref.wscale_expert_ffn = saved
