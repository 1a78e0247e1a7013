"""GPU tests of the single-launch deterministic gate (k_gate_fused):
MFMA logits over the whole K inside one block, last-arriver placement.

All cases use seed 47 and the run_pair input recipe with P = 128. For
exactly these inputs the smallest gap between a selected and an
unselected logit is at least 3.5e-3 (case C) against an fp32
summation-order error of at most 3.3e-5 (case D), so routing is compared
exactly and no token is excluded.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_parity import (assert_values, fresh_moe,  # noqa: F401
                                   make_cfg, routing_from_lib, run_pair)

pytestmark = pytest.mark.gpu


def _cfg(S, H, E, k, CF, dtype=2):
    return make_cfg(sequence_len=S, hidden_size=H, intermediate_size=128,
                    num_experts=E, expert_top_k=k, capacity_factor=CF,
                    torch_dtype=dtype)


def _ec(S, E, k, CF):
    return -(-S // E) * CF * k


# (S, H, E, k, CF, dtype): one tile, overflow; H = 64 leaves two of the
# four K-range waves without work
SINGLE_TILE = {
    "A": (128, 64, 8, 2, 1, 2),
    "A16": (128, 64, 8, 2, 1, 3),
    "F": (128, 64, 16, 1, 1, 2),
}


@pytest.mark.parametrize("case", sorted(SINGLE_TILE))
def test_single_tile_overflow_exact_lists(fresh_moe, case):
    S, H, E, k, CF, dtype = SINGLE_TILE[case]
    cfg, path = _cfg(S, H, E, k, CF, dtype)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    EC = _ec(S, E, k, CF)
    assert int(ref["eC"].max()) > EC, "case is meant to overflow"
    counts, tok, _ = routing_from_lib(E, EC)
    assert np.array_equal(counts.astype(np.int64), np.minimum(ref["eC"], EC))
    for e in range(E):
        assert np.array_equal(tok[e, : counts[e]].astype(np.int64),
                              ref["token_lists"][e]), f"expert {e} token list"
    # fp16 at the bf16 bar, as test_single_tile_fp16_top2 does
    assert_values(gate_out, ref["gate_out"], "bf16", "gate_out")
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def _check_multi_tile_routing(ref, counts, tok, E):
    want = ref["eC"].astype(np.int64)
    got = counts.astype(np.int64)
    assert np.array_equal(np.sort(got), np.sort(want))
    assert np.array_equal(got, want)
    for e in range(E):
        lst = tok[e, : counts[e]].astype(np.int64)
        assert np.array_equal(np.sort(lst),
                              np.sort(np.asarray(ref["token_lists"][e],
                                                 dtype=np.int64))), (
            f"expert {e} token set")
        # last-arriver placement: the tokens of one 128-token tile form
        # one contiguous, ascending run
        tiles = lst // 128
        runs = tiles[np.r_[True, tiles[1:] != tiles[:-1]]]
        assert len(np.unique(runs)) == len(runs), f"expert {e}: split tile run"
        same = tiles[1:] == tiles[:-1]
        assert np.all(lst[1:][same] > lst[:-1][same]), (
            f"expert {e}: tile run not ascending")


# multi-tile, no overflow: E not a multiple of 16 with a K remainder
# (H = 192: 6 steps over 4 waves), and E = 64 with k = 8
MULTI_TILE = {
    "B": (384, 192, 24, 3, 2),
    "C": (256, 128, 64, 8, 2),
}


@pytest.mark.parametrize("case", sorted(MULTI_TILE))
def test_multi_tile_placement(fresh_moe, case):
    S, H, E, k, CF = MULTI_TILE[case]
    cfg, path = _cfg(S, H, E, k, CF)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    EC = _ec(S, E, k, CF)
    assert int(ref["eC"].max()) <= EC, "case is meant not to overflow"
    counts, tok, _ = routing_from_lib(E, EC)
    _check_multi_tile_routing(ref, counts, tok, E)
    assert_values(gate_out, ref["gate_out"], "bf16", "gate_out")
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_repeat_calls_bit_identical(fresh_moe):
    """Case D (all four K-range waves busy at H = 1024, 4 tiles): five
    forwards on the same tensors - ticket words re-initialise themselves,
    the captured graph replays, and nothing depends on arrival order."""
    from flashmoe_amd.config import torch_dtype_of

    S, H, E, k, CF = 512, 1024, 8, 2, 2
    cfg, path = _cfg(S, H, E, k, CF)
    out0, gate0, ref, _ = run_pair(fresh_moe, cfg, path)
    EC = _ec(S, E, k, CF)
    assert int(ref["eC"].max()) <= EC
    dt = torch_dtype_of(2)
    g = torch.Generator(device="cpu").manual_seed(47)
    x = torch.randn(1, S, H, generator=g).to(dt).cuda()
    gw = torch.randn(H, E, generator=g).to(dt).cuda()
    ew = torch.randn(E, 2, 128, H, generator=g).to(dt).cuda()
    gates, outs, cnts = [gate0], [out0.clone()], []
    for _ in range(5):
        out = fresh_moe.moe_forward(x, gw, ew).clone()
        gates.append(fresh_moe.gate_output().clone())
        torch.cuda.synchronize()
        outs.append(out.view(S, H))
        cnts.append(routing_from_lib(E, EC)[0].astype(np.int64))
    for i in range(1, len(gates)):
        assert torch.equal(gates[i], gates[0]), f"gate_out differs on call {i}"
        assert torch.equal(outs[i], outs[0]), f"moe_out differs on call {i}"
    for i, c in enumerate(cnts):
        assert np.array_equal(c, ref["eC"].astype(np.int64)), f"counts, call {i}"


def test_knob_selects_old_path(fresh_moe):
    """FM_GATE_FUSED=0 forces the two-kernel gate; both gates route case B
    identically and agree on gate_out within the bf16 bar."""
    S, H, E, k, CF = MULTI_TILE["B"]
    EC = _ec(S, E, k, CF)
    res = {}
    try:
        for tag in ("old", "new"):
            if tag == "old":
                os.environ["FM_GATE_FUSED"] = "0"
            else:
                os.environ.pop("FM_GATE_FUSED", None)
            cfg, path = _cfg(S, H, E, k, CF)
            _, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
            counts, tok, _ = routing_from_lib(E, EC)
            res[tag] = (gate_out, counts.astype(np.int64),
                        [np.sort(tok[e, : counts[e]]) for e in range(E)])
            assert np.array_equal(res[tag][1], ref["eC"].astype(np.int64))
            fresh_moe.finalize()
    finally:
        os.environ.pop("FM_GATE_FUSED", None)
    assert np.array_equal(res["old"][1], res["new"][1])
    for e in range(E):
        assert np.array_equal(res["old"][2][e], res["new"][2][e]), (
            f"expert {e} token set")
    assert_values(res["new"][0], res["old"][0].float().cpu().numpy(), "bf16",
                  "gate_out new vs old")
