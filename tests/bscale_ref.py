"""CPU reference for 128x128 block scales of fp8 expert weights (torch_dtype
4, fm_set_weight_block_scales).

    W_eff[r, c] = float(W_fp8[r, c]) * s[r // 128][c // 128]

It is tests/wscale_ref.py's forward with one difference: every expert matmul
runs in float64 on W_eff = W * kron(s, ones(128, 128)). The kernels promote
fp32 partial sums per K block and round nothing that the unscaled path does
not round, so a plain high-precision matmul is the reference.

`scales` is [E + n_shared, BSC]; with PB = P / 128 and HB = H / 128 a record is
[s_up (PB x HB) | s_dn (HB x PB) | s_glu (PB x HB, gated only)], each part
row-major as [output block, K block]; shared experts last.

Rounding and activations are imported from oracle.moe_oracle / tests.gated_ref;
gate, routing, the expert loop and the combine are wscale_ref's.
"""
import numpy as np

from oracle.moe_oracle import _act, _elem_round
from tests import wscale_ref
from tests.gated_ref import gating_act

B = 128


def split_record(rec, P, H, gated):
    """(s_up [PB, HB], s_dn [HB, PB], s_glu [PB, HB] or None) of one record."""
    PB, HB = P // B, H // B
    n = PB * HB
    rec = np.asarray(rec, dtype=np.float32)
    assert rec.shape == ((3 if gated else 2) * n,)
    return (rec[:n].reshape(PB, HB), rec[n:2 * n].reshape(HB, PB),
            rec[2 * n:].reshape(PB, HB) if gated else None)


def w_eff(w, s):
    """float64 W * kron(s, ones(128, 128))."""
    return w.astype(np.float64) * np.kron(s.astype(np.float64), np.ones((B, B)))


def bscale_expert_ffn(rows, w, rec, cfg, b_up=None, b_dn=None):
    """One expert's FFN over rows [n, H]. w: the expert's [mats, P, H] slabs
    (slot 0 Wup, slot 1 the down buffer used as [H, P], slot 2 Wglu); rec: its
    block-scale record. fp32 result [n, H]."""
    gated = cfg.hidden_act >= 2
    P, H = w[0].shape
    s_up, s_dn, s_glu = split_record(rec, P, H, gated)
    a = rows.astype(np.float64)
    u = (a @ w_eff(w[0], s_up).T).astype(np.float32)
    if gated:
        assert b_up is None, "gated experts carry no b_up"
        g = (a @ w_eff(w[2], s_glu).T).astype(np.float32)
        y = gating_act(g, cfg.hidden_act) * u
    else:
        if b_up is not None:
            u = u + b_up.astype(np.float32)
        y = _act(u, cfg.hidden_act)
    y = _elem_round(y, cfg.element)
    z = (y.astype(np.float64) @ w_eff(w[1].reshape(H, P), s_dn).T).astype(
        np.float32)
    if b_dn is not None:
        z = z + b_dn.astype(np.float32)
    return z


def bscale_moe_forward(x, gate_w_buffer, expert_w, cfg, scales, n_shared=0,
                       b_up=None, b_dn=None):
    """wscale_ref.wscale_moe_forward with block-scale records: its forward,
    with bscale_expert_ffn in the place of its expert FFN."""
    saved = wscale_ref.wscale_expert_ffn
    wscale_ref.wscale_expert_ffn = bscale_expert_ffn
    try:
        return wscale_ref.wscale_moe_forward(x, gate_w_buffer, expert_w, cfg,
                                             scales, n_shared, b_up, b_dn)
    finally:
        wscale_ref.wscale_expert_ffn = saved
