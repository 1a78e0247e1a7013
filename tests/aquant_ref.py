"""CPU reference for fp8 activations on torch_dtype 4
(fm_set_activation_quant(1), "group128"). A row v is
quantised in groups of 128 along K, all in fp32:

    amax = max|v|;  s = amax / 448 (1 for a zero group);  q = e4m3_rne(v / s)

and both expert GEMMs see q * s in the place of the activation: x ahead of the
up GEMM, the bf16-rounded intermediate ahead of the down GEMM, in float64.
Weight scales: "block" records as in tests/bscale_ref.py, "channel" records as
in tests/wscale_ref.py (all ones = none). Gate, routing, the expert loop and
the combine are wscale_ref's (with kept lists: forward_given_kept's).
"""
import numpy as np

from oracle.moe_oracle import _act, _elem_round, e4m3_round
from tests import bscale_ref, routing_craft, wscale_ref
from tests.gated_ref import gating_act

G = 128


def quant_g128(a):
    """(q [n, K] fp32 on the e4m3 grid, s [n, K / 128] fp32) of rows a."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    n, K = a.shape
    g = a.reshape(n, K // G, G)
    amax = np.abs(g).max(axis=2)
    s = np.where(amax > 0, amax / np.float32(448.0),
                 np.float32(1.0)).astype(np.float32)
    q = e4m3_round((g / s[:, :, None]).astype(np.float32))
    return q.reshape(n, K), s


def dequant(a, quant=True):
    """float64 q * s of rows a; the rows themselves with quant off."""
    if not quant:
        return a.astype(np.float64)
    q, s = quant_g128(a)
    return q.astype(np.float64) * np.repeat(s.astype(np.float64), G, axis=1)


def make_expert_ffn(kind, quant=True):
    """wscale_expert_ffn's signature with both activation tensors quantised.
    kind "block": with quant off this is bscale_ref.bscale_expert_ffn."""
    def ffn(rows, w, rec, cfg, b_up=None, b_dn=None):
        gated = cfg.hidden_act >= 2
        P, H = w[0].shape
        if kind == "block":
            s_up, s_dn, s_glu = bscale_ref.split_record(rec, P, H, gated)
            w_up, w_dn = bscale_ref.w_eff(w[0], s_up), bscale_ref.w_eff(
                w[1].reshape(H, P), s_dn)
            w_glu = bscale_ref.w_eff(w[2], s_glu) if gated else None
            c_up = c_dn = c_glu = np.float32(1.0)
        else:
            c_up, c_dn, c_glu = wscale_ref.split_record(rec, P, H, gated)
            w_up, w_dn = w[0].astype(np.float64), w[1].reshape(H, P).astype(
                np.float64)
            w_glu = w[2].astype(np.float64) if gated else None
        a = dequant(rows, quant)
        u = (a @ w_up.T).astype(np.float32) * c_up
        if gated:
            assert b_up is None, "gated experts carry no b_up"
            g = (a @ w_glu.T).astype(np.float32) * c_glu
            y = gating_act(g, cfg.hidden_act) * u
        else:
            if b_up is not None:
                u = u + b_up.astype(np.float32)
            y = _act(u, cfg.hidden_act)
        y = _elem_round(y, cfg.element)
        z = (dequant(y, quant) @ w_dn.T).astype(np.float32) * c_dn
        if b_dn is not None:
            z = z + b_dn.astype(np.float32)
        return z.astype(np.float32)
    return ffn


def aquant_moe_forward(x, gate_w_buffer, expert_w, cfg, scales, kind,
                       n_shared=0, b_up=None, b_dn=None, quant=True,
                       kept_lists=None):
    """wscale_ref.wscale_moe_forward (routing_craft.forward_given_kept when
    kept_lists is given) with make_expert_ffn(kind, quant) as its expert FFN."""
    mod = wscale_ref if kept_lists is None else routing_craft
    saved = mod.wscale_expert_ffn
    mod.wscale_expert_ffn = make_expert_ffn(kind, quant)
    try:
        if kept_lists is None:
            return wscale_ref.wscale_moe_forward(
                x, gate_w_buffer, expert_w, cfg, scales, n_shared, b_up, b_dn)
        return routing_craft.forward_given_kept(
            x, gate_w_buffer, expert_w, cfg, kept_lists, n_shared, b_up, b_dn,
            scales)
    finally:
        mod.wscale_expert_ffn = saved
