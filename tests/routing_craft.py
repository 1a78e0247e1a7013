"""Inputs whose routing is prescribed exactly, and the forward conditioned on
a given kept set. Plain helpers for tests/test_loads_cpu.py and
tests/test_gpu_loads.py (no fixtures).

Crafted routing. The flat gate buffer, viewed [E, H] as the kernels and the
oracle view it, is the identity on the first E features, and x[:, :E] holds the
logits the test wants: every logit is ONE non-zero product, so it is the same
bit pattern under every summation order (MFMA gate, split-K atomics, the fp32
kernel, numpy). All logits are multiples of 1/8 in [-4, 4], exact in bf16 and
fp16: selected slot j carries 2.0 - 0.25 * j, every unselected expert a value
<= -2.0, so the k-th selected expert leads every unselected one by >= 1.0 (for
k <= 8) and no near-tie escape is needed. The top-k weights are far from
one-hot (last slot ~0.44 of the selected mass at k = 2, ~0.17 at k = 4), so an
error confined to a non-first slot is not hidden under the absolute bar.

THESE INPUTS DO NOT EXERCISE THE LOGITS GEMM NUMERICALLY: it multiplies by an
identity. The random-gate tests (test_gpu_parity, test_gpu_gate_fused,
test_gpu_router, ...) do that; these inputs place per-expert row counts on
tile and capacity edges, which random routing never does.

Kept-set-conditional reference. Under capacity overflow with more than one
128-token tile the kept SET depends on the block order, in the reference
implementation too. forward_given_kept is tests.wscale_ref.wscale_moe_forward
with route_tokens replaced by the caller's per-expert kept lists (read back
from the kernel with fm_read_routing): given that set the values are exact,
and check_kept asserts that the set is a legal one.
"""
import numpy as np

from oracle.moe_oracle import _elem_round, gate_forward
from tests.wscale_ref import wscale_expert_ffn

TORCH_DTYPE = {"fp32": "float32", "bf16": "bfloat16", "fp16": "float16"}
LAYOUTS = ("spread", "blocked")

# The load patterns of tests/test_gpu_loads.py (tests/test_loads_cpu.py checks
# each one on the CPU). S tokens, E experts, top-k, count vectors.
LOADS = {
    # tile edges, nothing dropped (BM = 128 and 256)
    "L": dict(S=512, E=4, k=2, counts=[
        (512, 256, 255, 1),    # full tile, full-minus-one, one row
        (129, 383, 257, 255),  # one past 128 and 256, one short of 256 and 384
        (127, 385, 128, 384),  # one short of 128, exact 128 and 384
        (512, 512, 0, 0),      # empty experts last
        (0, 512, 0, 512)]),    # empty expert first
    "L_top1": dict(S=512, E=4, k=1, counts=[(257, 255, 0, 0),
                                            (1, 127, 128, 256)]),
    "L_top3": dict(S=512, E=4, k=3, counts=[(512, 512, 511, 1)]),
    # capacity edges at CF = 1: EC = 256
    "O": dict(S=512, E=4, k=2, counts=[
        (512, 256, 255, 1),    # overflow by 256, exactly at capacity, one under
        (257, 511, 128, 128),  # overflow by one
        (512, 512, 0, 0)]),    # every token selects both overflowing experts
    # top-1 at CF = 1: EC = 128
    "O_top1": dict(S=512, E=4, k=1, counts=[(257, 127, 128, 0),
                                            (129, 128, 127, 128)]),
    # EC = 96 is no multiple of 128, pEC = 128
    "O8": dict(S=384, E=8, k=2, counts=[(97, 96, 95, 0, 120, 120, 120, 120)]),
    # decode sizes: the 32-row passes of k_decode_ffn
    "D": dict(S=96, E=4, k=2, counts=[(33, 32, 31, 96), (0, 96, 64, 32)]),
    "D1": dict(S=1, E=8, k=2, counts=[(1, 1, 0, 0, 0, 0, 0, 0)]),
    "D5": dict(S=5, E=8, k=2, counts=[(5, 5, 0, 0, 0, 0, 0, 0)]),
}


def patterns(name):
    """[(counts, layout, seed)] of LOADS[name]: every vector in both layouts,
    each with its own seed."""
    return [(c, lay, 100 * i + j)
            for i, c in enumerate(LOADS[name]["counts"])
            for j, lay in enumerate(LAYOUTS)]


def loads_to_sel(S, E, k, counts, layout, seed):
    """A [S, k] int32 selection (distinct experts per token, rank order) in
    which expert e is selected by exactly counts[e] tokens.

    The experts are laid out as runs of counts[e] along S * k positions and
    position p belongs to token p % S: a run is at most S long, so it never
    meets a token twice. layout "blocked" keeps that assignment - each
    expert's tokens are contiguous (cyclically: a run that passes S - 1 goes
    on at token 0); "spread" renames the tokens by a seeded permutation, so
    every expert's tokens cross the 128-token tiles. The rank order within a
    token is a seeded shuffle in both layouts."""
    counts = np.asarray(counts, dtype=np.int64)
    if counts.shape != (E,) or (counts < 0).any():
        raise ValueError(f"counts must be {E} non-negative integers")
    if int(counts.sum()) != S * k:
        raise ValueError(f"counts sum to {int(counts.sum())}, not S*k = {S * k}")
    if int(counts.max()) > S:
        raise ValueError(f"an expert cannot be selected by more than S = {S} "
                         f"tokens (max count {int(counts.max())})")
    if layout not in ("spread", "blocked"):
        raise ValueError(f"unknown layout {layout!r}")
    rng = np.random.RandomState(seed)
    runs = np.repeat(np.arange(E, dtype=np.int32), counts)  # [S * k]
    sel = np.ascontiguousarray(runs.reshape(k, S).T)        # token p % S
    for t in range(S):
        sel[t] = sel[t, rng.permutation(k)]
    if layout == "spread":
        sel = sel[rng.permutation(S)]
    assert all(len(set(row)) == k for row in sel.tolist())
    return sel


def craft_inputs(S, H, E, sel, element, seed):
    """(x [S, H], gate_w [H, E]) torch CPU tensors in the element's dtype
    for which the oracle's topk_idx equals sel (module docstring)."""
    import torch

    sel = np.asarray(sel)
    k = sel.shape[1]
    if H < E:
        raise ValueError(f"crafted routing needs H >= E (H {H}, E {E})")
    assert sel.shape == (S, k) and 1 <= k <= 8 and k <= E
    rng = np.random.RandomState(seed)
    x = rng.randn(S, H).astype(np.float32)
    # unselected: multiples of 1/8 in [-4, -2]
    logits = rng.randint(-32, -15, size=(S, E)).astype(np.float32) / 8.0
    for j in range(k):
        logits[np.arange(S), sel[:, j]] = 2.0 - 0.25 * j
    x[:, :E] = logits
    flat = np.zeros((E, H), dtype=np.float32)  # the buffer as used: [E, H]
    flat[np.arange(E), np.arange(E)] = 1.0
    dt = getattr(torch, TORCH_DTYPE[element])
    return (torch.from_numpy(x).to(dt),
            torch.from_numpy(flat.reshape(H, E).copy()).to(dt))


def forward_given_kept(x, gate_w, expert_w, cfg, kept_lists, n_shared=0,
                       b_up=None, b_dn=None, scales=None):
    """tests.wscale_ref.wscale_moe_forward with the routing given: expert e
    processes exactly the tokens kept_lists[e]. x [S, H], gate_w the flat gate
    buffer, expert_w [E + n_shared, mats, P, H], all fp32 numpy; cfg the
    OracleConfig of the routed experts; scales [E + n_shared, SC] or None
    (all ones: the plain, gated and shared references exactly). The combine
    weight stays gate_out[t, e] / mCw[t] with mCw over ALL selected experts -
    the reference does not renormalise over the kept slots."""
    S, H = x.shape
    E, k = cfg.num_experts, cfg.expert_top_k
    gated = cfg.hidden_act >= 2
    mats = 3 if gated else 2
    assert expert_w.shape[0] == E + n_shared and expert_w.shape[1] == mats
    P = expert_w.shape[2]
    if scales is None:
        scales = np.ones((E + n_shared, P + H + (P if gated else 0)),
                         dtype=np.float32)
    scales = np.asarray(scales, dtype=np.float32)
    assert scales.shape[0] == E + n_shared and len(kept_lists) == E
    x = _elem_round(x, cfg.element)
    gate_w = _elem_round(
        np.ascontiguousarray(gate_w, dtype=np.float32).reshape(E, H),
        cfg.element)
    expert_w = _elem_round(
        np.ascontiguousarray(expert_w, dtype=np.float32), cfg.element)

    gate_out, topk_idx, mCw, tie_margin = gate_forward(x, gate_w, cfg)

    def ffn(rows, e):
        return wscale_expert_ffn(
            rows, expert_w[e], scales[e], cfg,
            b_up[e] if b_up is not None else None,
            b_dn[e] if b_dn is not None else None)

    out = np.zeros((S, H), dtype=np.float32)
    for e in range(E):
        toks = np.asarray(kept_lists[e], dtype=np.int64)
        if len(toks) == 0:
            continue
        z = ffn(x[toks], e)
        if k > 1:
            scale = gate_out[toks, e].astype(np.float32) / mCw[toks]
            np.add.at(out, toks, _elem_round(z * scale[:, None], cfg.element))
        else:
            out[toks] = _elem_round(z, cfg.element)
    shared = np.zeros((S, H), dtype=np.float32)
    for s in range(n_shared):
        term = _elem_round(ffn(x, E + s), cfg.element)
        out = out + term
        shared = shared + term
    return {"gate_out": gate_out, "moe_out": _elem_round(out, cfg.element),
            "shared_out": shared, "topk_idx": topk_idx, "mCw": mCw,
            "eC": np.bincount(topk_idx.reshape(-1), minlength=E).astype(
                np.int64),
            "tie_margin": tie_margin}


def selectors(topk_idx, e):
    """The tokens that select expert e, in token order."""
    return np.nonzero((np.asarray(topk_idx) == e).any(axis=1))[0]


def check_kept(counts, tok, ref, EC):
    """The kernel's kept set (counts [E], tok [E, EC] from fm_read_routing) is
    a legal one for the reference's selection ref["topk_idx"] / ref["eC"]:
    counts[e] == min(eC[e], EC); no token twice in an expert's list; every
    listed token selects that expert; and with a single routing tile
    (S <= 128) the list is the oracle's: token order, clipped to EC."""
    sel = np.asarray(ref["topk_idx"])
    S = sel.shape[0]
    eC = np.asarray(ref["eC"], dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    want = np.minimum(eC, EC)
    assert np.array_equal(counts, want), f"routed counts {counts} != {want}"
    for e in range(len(eC)):
        got = np.asarray(tok[e, :counts[e]], dtype=np.int64)
        assert len(np.unique(got)) == len(got), f"expert {e}: token listed twice"
        who = selectors(sel, e)
        stray = np.setdiff1d(got, who)
        assert stray.size == 0, \
            f"expert {e}: tokens {stray[:8]} do not select it"
        if S <= 128:
            assert np.array_equal(got, who[:EC]), f"expert {e}: token order"


def kept_lists_of(counts, tok):
    """fm_read_routing's arrays as per-expert lists, each sorted (the order
    within an expert does not enter the values)."""
    return [np.sort(np.asarray(tok[e, :int(counts[e])], dtype=np.int64))
            for e in range(len(counts))]


def wholly_dropped(S, kept_lists):
    """Bool [S]: tokens that appear in no expert's kept list."""
    seen = np.zeros(S, dtype=bool)
    for toks in kept_lists:
        seen[np.asarray(toks, dtype=np.int64)] = True
    return ~seen
