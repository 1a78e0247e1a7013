"""CPU reference for shared experts (config key num_shared_experts).

    moe_out[t] = Element( sum_{j<k, kept[t,j]} Element(scale_j * FFN_{e_j}(x_t))
                        + sum_{s<nSh} Element(FFN_{E+s}(x_t)) )

The routed terms are those of oracle.moe_forward (plain experts) /
tests.gated_ref.gated_moe_forward (gated experts): scaled by
gate_out / probSum for k > 1, unscaled for k == 1, each rounded to Element.
A shared expert is an FFN over EVERY token with scale 1, always kept - a
token whose routed slots were all dropped still receives it. The sum is
fp32: routed terms first (added per expert as the two restated loops do),
then the shared ones in order s; one final rounding.

Expert weights are [E + nSh, mats, P, H] with the shared slabs last, b_dn
[E + nSh, H] when given.

Gate, routing, rounding and the two FFNs are imported; only the expert
loop and the combine are restated, with the shared terms added.
"""
import numpy as np

from oracle.moe_oracle import (_elem_round, expert_ffn, gate_forward,
                               route_tokens)
from tests.gated_ref import gated_expert_ffn


def _ffn(rows, w, hidden_act, cfg, b_dn):
    """One expert's FFN over rows; w is the expert's [mats, P, H] slabs."""
    if hidden_act >= 2:
        return gated_expert_ffn(rows, w[0], w[1].reshape(-1), w[2],
                                hidden_act, cfg.element, b_dn).astype(
                                    np.float32)
    return expert_ffn(rows, w[0], w[1].reshape(-1), None, b_dn, cfg)


def shared_moe_forward(x, gate_w_buffer, expert_w, cfg, n_shared, b_dn=None):
    """cfg: OracleConfig of the ROUTED experts (num_experts = E).
    expert_w: [E + n_shared, mats, P, H]. Returns the dict keys of
    oracle.moe_forward plus "shared_out", the fp32 sum of the rounded
    shared terms alone."""
    S, H = x.shape
    E, k = cfg.num_experts, cfg.expert_top_k
    mats = 3 if cfg.hidden_act >= 2 else 2
    assert expert_w.shape[0] == E + n_shared and expert_w.shape[1] == mats
    x = _elem_round(x, cfg.element)
    gate_w = _elem_round(
        np.ascontiguousarray(gate_w_buffer, dtype=np.float32).reshape(E, H),
        cfg.element)
    expert_w = _elem_round(
        np.ascontiguousarray(expert_w, dtype=np.float32), cfg.element)

    gate_out, topk_idx, mCw, tie_margin = gate_forward(x, gate_w, cfg)
    lists, eC, kept = route_tokens(topk_idx, cfg, S)

    out = np.zeros((S, H), dtype=np.float32)
    for e in range(E):
        toks = lists[e]
        if len(toks) == 0:
            continue
        z = _ffn(x[toks], expert_w[e], cfg.hidden_act, cfg,
                 b_dn[e] if b_dn is not None else None)
        if k > 1:
            scale = gate_out[toks, e].astype(np.float32) / mCw[toks]
            np.add.at(out, toks, _elem_round(z * scale[:, None], cfg.element))
        else:
            out[toks] = _elem_round(z, cfg.element)

    shared = np.zeros((S, H), dtype=np.float32)
    for s in range(n_shared):
        z = _ffn(x, expert_w[E + s], cfg.hidden_act, cfg,
                 b_dn[E + s] if b_dn is not None else None)
        term = _elem_round(z, cfg.element)
        out = out + term
        shared = shared + term
    return {"gate_out": gate_out, "moe_out": _elem_round(out, cfg.element),
            "shared_out": shared, "topk_idx": topk_idx, "eC": eC, "mCw": mCw,
            "tie_margin": tie_margin, "token_lists": lists, "kept": kept}
