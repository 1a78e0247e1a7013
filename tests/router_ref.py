"""CPU reference for the router variants (fm_router_config, DESIGN.md
par.5j): sigmoid scoring, a selection bias, group-limited top-k,
unnormalised and scaled weights.

For a token with fp32 logits l[e] = x_t . gate_w[e]:

    s[e] = softmax(l)[e]  (scoring_func 0)  |  1 / (1 + exp(-l[e]))  (1)
    c[e] = s[e] + bias[e]            selection only, never the weights
    groups: n_group contiguous groups of E / n_group; a group's score is
            max c (group_score 0) or the sum of its two largest c (1); the
            topk_group best groups are kept by iterative strict->
            first-index argmax; experts of other groups cannot be selected
    top-k:  iterative strict-> first-index argmax over c, k times
    mCw   = sum_j s[e_j] in selection order
    D     = (norm_topk_prob ? mCw : 1.0f) / routed_scaling_factor   (fp32)
    weight of selection j = Element(s[e_j]) / D;  gate_out = Element(s)

With softmax, no bias and group_score 0 the selection score is monotone in
the logits and selection runs on the logits, as oracle.gate_forward does:
with every key at its default this module IS oracle.moe_forward.

Rounding helpers, route_tokens and the expert FFNs come from
oracle.moe_oracle, tests/gated_ref.py and tests/shared_ref.py; the gate
and the combine are restated here. Two margins are returned for the
near-tie escape of the GPU tests, both in units of c:
  margin_sel  c gap between the k-th selected and the best unselected
              allowed expert (inf when none is left)
  margin_grp  gap between the topk_group-th kept and the best dropped
              group score (inf without a group limit)
"""
import numpy as np

from oracle.moe_oracle import _elem_round, padded_experts, route_tokens
from tests.shared_ref import _ffn

ROUTER_DEFAULTS = dict(scoring_func=0, norm_topk_prob=1, n_group=1,
                       topk_group=1, group_score=0, routed_scaling_factor=1.0)


def _iter_argmax(v, n):
    """n rounds of first-index argmax with strict >, masking the winner.
    v: [S, M]. Returns idx [S, n] and the masked copy of v."""
    S = v.shape[0]
    masked = v.copy()
    idx = np.zeros((S, n), dtype=np.int32)
    for i in range(n):
        a = np.argmax(masked, axis=1)
        idx[:, i] = a
        masked[np.arange(S), a] = -np.inf
    return idx, masked


def router_gate_forward(x, gate_w, cfg, router=None, bias=None):
    """x [S, H] and gate_w [E, H] element-rounded. Returns a dict:
    gate_out [S, PX] (Element), topk_idx [S, k], mCw [S], D [S],
    margin_sel [S], margin_grp [S]."""
    r = dict(ROUTER_DEFAULTS, **(router or {}))
    S = x.shape[0]
    E, k = cfg.num_experts, cfg.expert_top_k
    G, TG = r["n_group"], r["topk_group"]
    logits = x.astype(np.float32) @ gate_w.astype(np.float32).T
    if r["scoring_func"] == 0:
        m = logits.max(axis=1, keepdims=True)
        ex = np.exp(logits - m, dtype=np.float32)
        s = ex / ex.sum(axis=1, keepdims=True, dtype=np.float32)
    else:
        s = (np.float32(1.0) /
             (np.float32(1.0) + np.exp(-logits, dtype=np.float32)))
    s = s.astype(np.float32)
    c = s if bias is None else (s + bias.astype(np.float32)[None, :])
    c = c.astype(np.float32)
    on_logits = (r["scoring_func"] == 0 and bias is None
                 and r["group_score"] == 0)
    v = logits if on_logits else c  # what the argmaxes compare

    allowed = np.ones((S, E), dtype=bool)
    margin_grp = np.full(S, np.inf, dtype=np.float32)
    if G > 1:
        gs = E // G

        def gscore(a):
            a = a.reshape(S, G, gs)
            if r["group_score"] == 0:
                return a.max(axis=2)
            top2 = -np.sort(-a, axis=2)[:, :, :2]
            return (top2[:, :, 0] + top2[:, :, 1]).astype(np.float32)

        gidx, _ = _iter_argmax(gscore(v), TG)
        keep = np.zeros((S, G), dtype=bool)
        keep[np.arange(S)[:, None], gidx] = True
        allowed = np.repeat(keep, gs, axis=1)
        if TG < G:
            gc = gscore(c)  # the margin is in units of c
            kept_min = np.where(keep, gc, np.inf).min(axis=1)
            drop_max = np.where(keep, -np.inf, gc).max(axis=1)
            margin_grp = (kept_min - drop_max).astype(np.float32)

    sel, _ = _iter_argmax(np.where(allowed, v, -np.inf), k)
    rows = np.arange(S)
    chosen = np.zeros((S, E), dtype=bool)
    chosen[rows[:, None], sel] = True
    rest = np.where(allowed & ~chosen, c, -np.inf).max(axis=1)
    margin_sel = (c[rows, sel[:, k - 1]] - rest).astype(np.float32)

    mCw = s[rows[:, None], sel].sum(axis=1, dtype=np.float32)
    num = mCw if r["norm_topk_prob"] else np.ones(S, dtype=np.float32)
    D = (num / np.float32(r["routed_scaling_factor"])).astype(np.float32)

    gate_out = np.zeros((S, padded_experts(E)), dtype=np.float32)
    gate_out[:, :E] = s
    return {"gate_out": _elem_round(gate_out, cfg.element), "topk_idx": sel,
            "mCw": mCw.astype(np.float32), "D": D,
            "margin_sel": margin_sel, "margin_grp": margin_grp}


def router_moe_forward(x, gate_w_buffer, expert_w, cfg, router=None,
                       bias=None, n_shared=0, b_dn=None):
    """oracle.moe_forward under a router variant. cfg: OracleConfig of the
    routed experts (hidden_act 0..3, mx_fp8 honoured); expert_w
    [E + n_shared, mats, P, H]. Returns the keys of oracle.moe_forward plus
    D, margin_sel and margin_grp."""
    S, H = x.shape
    E, k = cfg.num_experts, cfg.expert_top_k
    x = _elem_round(x, cfg.element)
    gate_w = _elem_round(
        np.ascontiguousarray(gate_w_buffer, dtype=np.float32).reshape(E, H),
        cfg.element)
    expert_w = _elem_round(
        np.ascontiguousarray(expert_w, dtype=np.float32), cfg.element)
    assert expert_w.shape[0] == E + n_shared

    gt = router_gate_forward(x, gate_w, cfg, router, bias)
    gate_out, D = gt["gate_out"], gt["D"]
    lists, eC, kept = route_tokens(gt["topk_idx"], cfg, S)

    out = np.zeros((S, H), dtype=np.float32)
    for e in range(E):
        toks = lists[e]
        if len(toks) == 0:
            continue
        z = _ffn(x[toks], expert_w[e], cfg.hidden_act, cfg,
                 b_dn[e] if b_dn is not None else None)
        if k > 1:
            scale = gate_out[toks, e].astype(np.float32) / D[toks]
            np.add.at(out, toks, _elem_round(z * scale[:, None], cfg.element))
        else:
            out[toks] = _elem_round(z, cfg.element)
    for sh in range(n_shared):
        z = _ffn(x, expert_w[E + sh], cfg.hidden_act, cfg,
                 b_dn[E + sh] if b_dn is not None else None)
        out = out + _elem_round(z, cfg.element)
    return {"gate_out": gate_out, "moe_out": _elem_round(out, cfg.element),
            "topk_idx": gt["topk_idx"], "eC": eC, "mCw": gt["mCw"],
            "D": D, "margin_sel": gt["margin_sel"],
            "margin_grp": gt["margin_grp"], "tie_margin": gt["margin_sel"],
            "token_lists": lists, "kept": kept}
