"""CPU reference for per-token fp8 activations on torch_dtype 4
(fm_set_activation_quant(2), "token"): tests/aquant_ref.py
with the group equal to the row, all in fp32:

    amax = max|v| over the row;  s = amax / 448 (1 for a zero row);
    q = e4m3_rne(v / s)

Both expert GEMMs see q * s in float64 in the place of the activation; the
weight scales are per-channel records (all ones = none). mode "group128" and
None give aquant_ref's quantised and unquantised forwards over the same
records, for comparison.
"""
import numpy as np

from oracle.moe_oracle import e4m3_round
from tests import aquant_ref, routing_craft, wscale_ref


def quant_row(a):
    """(q [n, K] fp32 on the e4m3 grid, s [n] fp32) of rows a."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    amax = np.abs(a).max(axis=1)
    s = np.where(amax > 0, amax / np.float32(448.0),
                 np.float32(1.0)).astype(np.float32)
    return e4m3_round((a / s[:, None]).astype(np.float32)), s


def dequant(a, quant=True):
    if not quant:
        return a.astype(np.float64)
    q, s = quant_row(a)
    return q.astype(np.float64) * s.astype(np.float64)[:, None]


def make_expert_ffn(mode="token"):
    """aquant_ref's per-channel expert FFN with `mode`'s quantiser."""
    if mode != "token":
        return aquant_ref.make_expert_ffn("channel", mode is not None)

    def ffn(*args, **kw):
        saved, aquant_ref.dequant = aquant_ref.dequant, dequant
        try:
            return aquant_ref.make_expert_ffn("channel")(*args, **kw)
        finally:
            aquant_ref.dequant = saved
    return ffn


def tquant_moe_forward(x, gate_w_buffer, expert_w, cfg, scales, n_shared=0,
                       b_up=None, b_dn=None, mode="token", kept_lists=None):
    """wscale_ref.wscale_moe_forward (routing_craft.forward_given_kept when
    kept_lists is given) with make_expert_ffn(mode) as its expert FFN."""
    mod = wscale_ref if kept_lists is None else routing_craft
    saved = mod.wscale_expert_ffn
    mod.wscale_expert_ffn = make_expert_ffn(mode)
    try:
        if kept_lists is None:
            return wscale_ref.wscale_moe_forward(
                x, gate_w_buffer, expert_w, cfg, scales, n_shared, b_up, b_dn)
        return routing_craft.forward_given_kept(
            x, gate_w_buffer, expert_w, cfg, kept_lists, n_shared, b_up, b_dn,
            scales)
    finally:
        mod.wscale_expert_ffn = saved
