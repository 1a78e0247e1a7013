"""CPU reference for per-output-channel weight scales of fp8 expert weights
(torch_dtype 4 and 5, fm_set_weight_scales).

    W_eff[r, :] = float(W_fp8[r, :]) * s[r]        r = output channel

The scale is applied TO THE fp32 MATMUL RESULT, per column, where the kernels
apply it - never by building W_eff and rounding it to the element type:

    up, ungated   y = Element(act((a @ Wup^T) * s_up + b_up))
    up, gated     y = Element(act((a @ Wglu^T) * s_glu) * ((a @ Wup^T) * s_up))
    down          z = (y @ Wdn^T) * s_dn + b_dn

`scales` is [E + n_shared, SC], SC = P + H (+ P gated), one record
[s_up (P) | s_dn (H) | s_glu (P)] per expert, shared experts last.

Gate, routing, rounding, activations and the MX activation quantisation are
imported from oracle.moe_oracle / tests.gated_ref; only the expert FFN, the
expert loop and the combine of oracle.moe_forward, gated_ref.gated_moe_forward
and shared_ref.shared_moe_forward are restated here. With all-ones scales
every result equals theirs exactly.
"""
import numpy as np

from oracle.moe_oracle import (_act, _elem_round, gate_forward, mx_quant_rows,
                               route_tokens)
from tests.gated_ref import gating_act


def split_record(rec, P, H, gated):
    """(s_up [P], s_dn [H], s_glu [P] or None) of one expert's record."""
    rec = np.asarray(rec, dtype=np.float32)
    assert rec.shape == (P + H + (P if gated else 0),)
    return rec[:P], rec[P:P + H], (rec[P + H:] if gated else None)


def wscale_expert_ffn(rows, w, rec, cfg, b_up=None, b_dn=None):
    """One expert's FFN over rows [n, H]. w: the expert's [mats, P, H] slabs
    (slot 0 Wup, slot 1 the down buffer used as [H, P], slot 2 Wglu); rec: its
    scale record. fp32 result [n, H]."""
    gated = cfg.hidden_act >= 2
    P, H = w[0].shape
    s_up, s_dn, s_glu = split_record(rec, P, H, gated)
    w = w.astype(np.float32)
    a_up = mx_quant_rows(rows) if cfg.mx_fp8 else rows.astype(np.float32)
    u = (a_up @ w[0].T) * s_up
    if gated:
        assert b_up is None, "gated experts carry no b_up"
        g = (a_up @ w[2].T) * s_glu
        y = gating_act(g, cfg.hidden_act) * u
    else:
        if b_up is not None:
            u = u + b_up.astype(np.float32)
        y = _act(u, cfg.hidden_act)
    y = _elem_round(y, cfg.element)
    a_dn = mx_quant_rows(y) if cfg.mx_fp8 else y
    z = (a_dn @ w[1].reshape(H, P).T) * s_dn
    if b_dn is not None:
        z = z + b_dn.astype(np.float32)
    return z.astype(np.float32)


def wscale_moe_forward(x, gate_w_buffer, expert_w, cfg, scales, n_shared=0,
                       b_up=None, b_dn=None):
    """The forward of oracle.moe_forward (plain experts), gated_moe_forward
    (cfg.hidden_act 2/3) and shared_moe_forward (n_shared > 0) with weight
    scales. cfg is the OracleConfig of the ROUTED experts; expert_w is
    [E + n_shared, mats, P, H]; b_up / b_dn are indexed like expert_w."""
    S, H = x.shape
    E, k = cfg.num_experts, cfg.expert_top_k
    mats = 3 if cfg.hidden_act >= 2 else 2
    assert expert_w.shape[0] == E + n_shared and expert_w.shape[1] == mats
    scales = np.asarray(scales, dtype=np.float32)
    assert scales.shape[0] == E + n_shared
    x = _elem_round(x, cfg.element)
    gate_w = _elem_round(
        np.ascontiguousarray(gate_w_buffer, dtype=np.float32).reshape(E, H),
        cfg.element)
    expert_w = _elem_round(
        np.ascontiguousarray(expert_w, dtype=np.float32), cfg.element)

    gate_out, topk_idx, mCw, tie_margin = gate_forward(x, gate_w, cfg)
    lists, eC, kept = route_tokens(topk_idx, cfg, S)

    def ffn(rows, e):
        return wscale_expert_ffn(
            rows, expert_w[e], scales[e], cfg,
            b_up[e] if b_up is not None else None,
            b_dn[e] if b_dn is not None else None)

    out = np.zeros((S, H), dtype=np.float32)
    for e in range(E):
        toks = lists[e]
        if len(toks) == 0:
            continue
        z = ffn(x[toks], e)
        if k > 1:
            scale = gate_out[toks, e].astype(np.float32) / mCw[toks]
            np.add.at(out, toks, _elem_round(z * scale[:, None], cfg.element))
        else:
            out[toks] = _elem_round(z, cfg.element)
    for s in range(n_shared):
        out = out + _elem_round(ffn(x, E + s), cfg.element)
    return {"gate_out": gate_out, "moe_out": _elem_round(out, cfg.element),
            "topk_idx": topk_idx, "eC": eC, "mCw": mCw,
            "tie_margin": tie_margin, "token_lists": lists, "kept": kept}
