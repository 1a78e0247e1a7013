"""CPU reference for gated experts (hidden_act 2 SwiGLU, 3 GeGLU).

    h = act(a @ Wglu^T) * (a @ Wup^T)   fp32, rounded ONCE to Element
    z = h @ Wdn^T (+ b_dn)

Expert weights are [E, 3, P, H]: slot 0 = Wup [P, H], slot 1 = the down
buffer (flat, used as [H, P]), slot 2 = Wglu [P, H].

Gate, routing and element rounding come from oracle.moe_oracle; only the
expert loop and the combine of oracle.moe_forward are re-stated here, with
the gated intermediate. Everything else follows moe_forward: inputs are
rounded to Element, k > 1 contributions are rounded after scaling, and
the output is rounded at the end.
"""
import numpy as np

from oracle.moe_oracle import _elem_round, gate_forward, route_tokens


def gating_act(v: np.ndarray, hidden_act: int) -> np.ndarray:
    if hidden_act == 2:  # silu(v) = v / (1 + exp(-v))
        return v / (1.0 + np.exp(-v))
    if hidden_act == 3:  # exact-erf gelu
        from scipy.special import erf

        return 0.5 * v * (1.0 + erf(v / np.sqrt(2.0).astype(v.dtype)))
    raise ValueError(f"hidden_act {hidden_act} is not gated")


def gated_expert_ffn(rows, w_up, w_dn_flat, w_glu, hidden_act, element,
                     b_dn=None, acc=np.float32):
    """rows [n, H]; w_up, w_glu [P, H]; w_dn_flat: P*H elements used as
    [H, P]. acc is the arithmetic type (float64 for error studies)."""
    P, H = w_up.shape
    a = rows.astype(acc)
    g = a @ w_glu.astype(acc).T
    u = a @ w_up.astype(acc).T
    y = _elem_round(gating_act(g, hidden_act) * u, element).astype(acc)
    z = y @ w_dn_flat.reshape(H, P).astype(acc).T
    if b_dn is not None:
        z = z + b_dn.astype(acc)
    return z


def gated_moe_forward(x, gate_w_buffer, expert_w, cfg, b_dn=None,
                      acc=np.float32):
    """oracle.moe_forward for cfg.hidden_act in {2, 3} and [E, 3, P, H]
    expert weights. Returns the same dict keys the tests use."""
    S, H = x.shape
    E, k = cfg.num_experts, cfg.expert_top_k
    assert expert_w.shape[1] == 3, "gated experts carry three [P, H] slabs"
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
        z = gated_expert_ffn(
            x[toks], expert_w[e, 0], expert_w[e, 1].reshape(-1),
            expert_w[e, 2], cfg.hidden_act, cfg.element,
            b_dn[e] if b_dn is not None else None, acc).astype(np.float32)
        if k > 1:
            scale = gate_out[toks, e].astype(np.float32) / mCw[toks]
            np.add.at(out, toks, _elem_round(z * scale[:, None], cfg.element))
        else:
            out[toks] = _elem_round(z, cfg.element)
    return {"gate_out": gate_out, "moe_out": _elem_round(out, cfg.element),
            "topk_idx": topk_idx, "eC": eC, "mCw": mCw,
            "tie_margin": tie_margin, "token_lists": lists, "kept": kept}
