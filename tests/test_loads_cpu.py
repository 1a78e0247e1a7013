"""tests/routing_craft.py on the CPU: the crafted inputs give exactly the
prescribed routing, forward_given_kept is the four references bit for bit
when fed the oracle's own kept lists, and it tells kept sets apart.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle.moe_oracle import (OracleConfig, e4m3_round, expert_capacity,
                               gate_forward, moe_forward as oracle_forward)
from tests.gated_ref import gated_moe_forward
from tests.routing_craft import (LAYOUTS, LOADS, check_kept, craft_inputs,
                                 forward_given_kept, loads_to_sel, patterns,
                                 selectors)
from tests.shared_ref import shared_moe_forward
from tests.test_gpu_parity import assert_values
from tests.wscale_ref import wscale_moe_forward


def np32(t):
    return t.float().numpy()


def weights(n, mats, P, H, seed=47, fp8=False):
    w = np.random.RandomState(seed).randn(n, mats, P, H).astype(np.float32)
    return e4m3_round(w) if fp8 else w


# --- the crafted inputs route as prescribed

@pytest.mark.parametrize("name", sorted(LOADS))
def test_crafted_routing_is_the_prescribed_one(name):
    S, E, k = (LOADS[name][key] for key in "SEk")
    H, P = 128, 64
    ew = weights(E, 2, P, H)
    for element in ("bf16", "fp16", "fp32"):
        ocfg = OracleConfig(num_experts=E, expert_top_k=k, capacity_factor=2,
                            drop_tokens=0, element=element)
        for counts, layout, seed in patterns(name):
            sel = loads_to_sel(S, E, k, counts, layout, seed)
            x, gw = craft_inputs(S, H, E, sel, element, seed)
            assert tuple(gw.shape) == (H, E)
            ref = oracle_forward(np32(x), np32(gw).reshape(-1), ew, ocfg)
            assert np.array_equal(ref["topk_idx"], sel), (counts, layout)
            assert float(ref["tie_margin"].min()) >= 1.0
            assert np.array_equal(ref["eC"], np.asarray(counts))
            if element != "bf16":
                break  # the other formats: one pattern each


def test_layouts():
    S, E, k = 512, 4, 2
    counts = (129, 383, 257, 255)
    blocked = loads_to_sel(S, E, k, counts, "blocked", 3)
    spread = loads_to_sel(S, E, k, counts, "spread", 3)
    for e in range(E):
        tb, ts = selectors(blocked, e), selectors(spread, e)
        assert len(tb) == len(ts) == counts[e]
        assert tb[-1] - tb[0] == counts[e] - 1            # contiguous
        assert len(set((ts // 128).tolist())) == S // 128  # every tile
    # both rank orders occur
    assert 0 < int((blocked[:, 0] < blocked[:, 1]).sum()) < S


@pytest.mark.parametrize("counts", [(512, 512, 1, 0), (513, 511, 0, 0),
                                    (512, 256, 255, 0), (600, 424, 0, 0),
                                    (512, 512, -1, 1), (512, 512, 0)])
def test_infeasible_loads_raise(counts):
    with pytest.raises(ValueError):
        loads_to_sel(512, 4, 2, counts, "spread", 0)


def test_unknown_layout_and_small_h_raise():
    with pytest.raises(ValueError):
        loads_to_sel(4, 2, 1, (2, 2), "striped", 0)
    sel = loads_to_sel(4, 8, 2, (4, 4, 0, 0, 0, 0, 0, 0), "blocked", 0)
    with pytest.raises(ValueError):
        craft_inputs(4, 4, 8, sel, "bf16", 0)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_last_slot_weight_is_not_negligible(k):
    """The reference's own combine weights on crafted inputs: the mean weight
    of the last selected slot is >= 0.1 (random unit-normal gates give a
    median of 0.0095 at H=128, E=8, k=2 and 3.7e-5 at E=16, k=4)."""
    S, E, H = 256, 8, 128
    counts = [S * k // E] * E
    sel = loads_to_sel(S, E, k, counts, "spread", 5)
    x, gw = craft_inputs(S, H, E, sel, "bf16", 5)
    ocfg = OracleConfig(num_experts=E, expert_top_k=k, element="bf16")
    gate_out, topk, mCw, _ = gate_forward(np32(x), np32(gw).reshape(E, H),
                                          ocfg)
    assert np.array_equal(topk, sel)
    last = gate_out[np.arange(S), sel[:, k - 1]] / mCw
    assert float(last.mean()) >= 0.1, float(last.mean())


@pytest.mark.parametrize("H,E,k,median_below,share_below", [
    (128, 8, 2, 2e-2, 0.3),     # median 0.0087, 24 % of the tokens above 0.1
    (128, 16, 4, 1e-4, 0.02),   # median 3.1e-5
    (1024, 8, 2, 1e-5, 0.15)])  # median 5.1e-7
def test_random_gates_are_close_to_one_hot(H, E, k, median_below, share_below):
    """The measurement the crafted inputs answer, recomputed: x and gate
    weights unit normal (logit standard deviation sqrt(H)), seed 47, bf16,
    S=512. The last selected slot's weight is tiny, so an error confined to
    it mostly sits under the absolute bar."""
    S = 512
    g = torch.Generator(device="cpu").manual_seed(47)
    x = torch.randn(1, S, H, generator=g).to(torch.bfloat16)
    gw = torch.randn(H, E, generator=g).to(torch.bfloat16)
    ocfg = OracleConfig(num_experts=E, expert_top_k=k, element="bf16")
    gate_out, sel, mCw, _ = gate_forward(
        np32(x).reshape(S, H), np32(gw).reshape(E, H), ocfg)
    last = gate_out[np.arange(S), sel[:, k - 1]] / mCw
    assert float(np.median(last)) < median_below
    assert float((last > 0.1).mean()) < share_below


# --- forward_given_kept is the four references, bit for bit

def random_case(E=8, k=2, S=256, H=128):
    g = torch.Generator(device="cpu").manual_seed(47)
    x = torch.randn(S, H, generator=g).to(torch.bfloat16)
    gw = torch.randn(H, E, generator=g).to(torch.bfloat16)
    return np32(x), np32(gw).reshape(-1)


def crafted_case(name="O", which=0, H=128):
    S, E, k = (LOADS[name][key] for key in "SEk")
    counts, layout, seed = patterns(name)[which]
    sel = loads_to_sel(S, E, k, counts, layout, seed)
    x, gw = craft_inputs(S, H, E, sel, "bf16", seed)
    return np32(x), np32(gw).reshape(-1)


CASES = {"random": (random_case, 8), "crafted": (crafted_case, 4)}


def same(a, b):
    for key in ("gate_out", "moe_out", "topk_idx", "eC", "mCw", "tie_margin"):
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("case", sorted(CASES))
def test_bit_equal_to_the_oracle(case):
    make, E = CASES[case]
    x, gw = make()
    H, P = x.shape[1], 128
    ew = weights(E, 2, P, H)
    rs = np.random.RandomState(1)
    b_up = rs.randn(E, P).astype(np.float32)
    b_dn = rs.randn(E, H).astype(np.float32)
    for act, biases in ((0, False), (1, True)):
        ocfg = OracleConfig(num_experts=E, expert_top_k=2, hidden_act=act,
                            element="bf16")
        kw = dict(b_up=b_up, b_dn=b_dn) if biases else {}
        want = oracle_forward(x, gw, ew, ocfg, **kw)
        assert int(want["eC"].sum()) > sum(map(len, want["token_lists"]))
        got = forward_given_kept(x, gw, ew, ocfg, want["token_lists"], **kw)
        same(got, want)


@pytest.mark.parametrize("case", sorted(CASES))
def test_bit_equal_to_the_gated_reference(case):
    make, E = CASES[case]
    x, gw = make()
    H, P = x.shape[1], 128
    ew = weights(E, 3, P, H)
    b_dn = np.random.RandomState(2).randn(E, H).astype(np.float32)
    ocfg = OracleConfig(num_experts=E, expert_top_k=2, hidden_act=2,
                        element="bf16")
    want = gated_moe_forward(x, gw, ew, ocfg, b_dn=b_dn)
    got = forward_given_kept(x, gw, ew, ocfg, want["token_lists"], b_dn=b_dn)
    same(got, want)


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("act", [0, 2])
def test_bit_equal_to_the_shared_reference(case, act):
    make, E = CASES[case]
    x, gw = make()
    H, P = x.shape[1], 128
    ew = weights(E + 2, 3 if act >= 2 else 2, P, H)
    ocfg = OracleConfig(num_experts=E, expert_top_k=2, hidden_act=act,
                        element="bf16")
    want = shared_moe_forward(x, gw, ew, ocfg, 2)
    got = forward_given_kept(x, gw, ew, ocfg, want["token_lists"], n_shared=2)
    same(got, want)
    assert np.array_equal(got["shared_out"], want["shared_out"])


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("act,mx", [(0, False), (2, False), (0, True)])
def test_bit_equal_to_the_weight_scale_reference(case, act, mx):
    make, E = CASES[case]
    x, gw = make()
    H, P = x.shape[1], 128
    gated = act >= 2
    ew = weights(E + 1, 3 if gated else 2, P, H, fp8=True)
    sc = np.exp2(np.random.RandomState(48).uniform(
        -2, 1, (E + 1, P + H + (P if gated else 0)))).astype(np.float32)
    ocfg = OracleConfig(num_experts=E, expert_top_k=2, hidden_act=act,
                        element="bf16", mx_fp8=mx)
    want = wscale_moe_forward(x, gw, ew, ocfg, sc, n_shared=1)
    got = forward_given_kept(x, gw, ew, ocfg, want["token_lists"], n_shared=1,
                             scales=sc)
    same(got, want)


def test_top1_bit_equal_and_check_kept_accepts_the_oracle():
    S, E, k = (LOADS["O_top1"][key] for key in "SEk")
    counts, layout, seed = patterns("O_top1")[0]
    sel = loads_to_sel(S, E, k, counts, layout, seed)
    x, gw = craft_inputs(S, 128, E, sel, "bf16", seed)
    x, gw = np32(x), np32(gw).reshape(-1)
    ew = weights(E, 2, 128, 128)
    ocfg = OracleConfig(num_experts=E, expert_top_k=1, element="bf16")
    want = oracle_forward(x, gw, ew, ocfg)
    got = forward_given_kept(x, gw, ew, ocfg, want["token_lists"])
    same(got, want)
    EC = expert_capacity(S, ocfg)
    assert EC == 128
    tok = np.zeros((E, EC), dtype=np.uint32)
    for e, toks in enumerate(want["token_lists"]):
        tok[e, :len(toks)] = toks
    check_kept(np.minimum(want["eC"], EC), tok, got, EC)


# --- check_kept

def small_routing():
    """One routing tile, drops: S=128, E=4, k=2, CF=1 -> EC = 64."""
    S, E, k = 128, 4, 2
    sel = loads_to_sel(S, E, k, (100, 64, 63, 29), "spread", 9)
    x, gw = craft_inputs(S, 128, E, sel, "bf16", 9)
    ocfg = OracleConfig(num_experts=E, expert_top_k=k, element="bf16")
    want = oracle_forward(np32(x), np32(gw).reshape(-1),
                          weights(E, 2, 64, 128), ocfg)
    EC = expert_capacity(S, ocfg)
    tok = np.zeros((E, EC), dtype=np.uint32)
    for e, toks in enumerate(want["token_lists"]):
        tok[e, :len(toks)] = toks
    return want, np.minimum(want["eC"], EC), tok, EC


def test_check_kept_single_tile():
    want, counts, tok, EC = small_routing()
    assert EC == 64 and counts.tolist() == [64, 64, 63, 29]
    check_kept(counts, tok, want, EC)
    bad = counts.copy()
    bad[0] -= 1
    with pytest.raises(AssertionError, match="routed counts"):
        check_kept(bad, tok, want, EC)
    dup = tok.copy()
    dup[1, 5] = dup[1, 4]
    with pytest.raises(AssertionError, match="twice"):
        check_kept(counts, dup, want, EC)
    stray = tok.copy()
    stray[3, 0] = np.setdiff1d(np.arange(128), selectors(want["topk_idx"], 3))[0]
    with pytest.raises(AssertionError, match="do not select"):
        check_kept(counts, stray, want, EC)
    # a legal set in another order: refused with one tile only
    swapped = tok.copy()
    dropped = selectors(want["topk_idx"], 0)[EC]
    swapped[0, EC - 1] = dropped
    with pytest.raises(AssertionError, match="token order"):
        check_kept(counts, swapped, want, EC)


# --- forward_given_kept tells kept sets apart

def test_one_kept_pair_moves_that_tokens_row_outside_the_bar():
    x, gw = crafted_case("O", 0)  # (512, 256, 255, 1), spread
    E, H, P = 4, 128, 256
    ew = weights(E, 2, P, H)
    ocfg = OracleConfig(num_experts=E, expert_top_k=2, element="bf16")
    base = oracle_forward(x, gw, ew, ocfg)
    lists = base["token_lists"]
    ref = forward_given_kept(x, gw, ew, ocfg, lists)["moe_out"]
    lost = np.setdiff1d(selectors(base["topk_idx"], 0), lists[0])
    assert len(lost) == 256
    rs = np.random.RandomState(4)
    for e in range(3):
        for i in rs.choice(len(lists[e]), 8, replace=False):
            t = int(lists[e][i])
            # the pair (t, e) removed
            cut = [l if j != e else np.delete(l, i)
                   for j, l in enumerate(lists)]
            got = forward_given_kept(x, gw, ew, ocfg, cut)["moe_out"]
            with pytest.raises(AssertionError):
                assert_values(torch.from_numpy(got), ref, "bf16", "moe_out")
            others = np.arange(len(ref)) != t
            assert np.array_equal(got[others], ref[others])
    for i, t2 in zip(rs.choice(256, 8, replace=False), lost[:8]):
        # another selector of expert 0 in its place: both rows move
        t = int(lists[0][i])
        swap = [l.copy() for l in lists]
        swap[0][i] = t2
        got = forward_given_kept(x, gw, ew, ocfg, swap)["moe_out"]
        others = ~np.isin(np.arange(len(ref)), [t, t2])
        assert np.array_equal(got[others], ref[others])
        for row in (t, int(t2)):
            only = ref.copy()
            only[row] = got[row]
            with pytest.raises(AssertionError):
                assert_values(torch.from_numpy(only), ref, "bf16", "moe_out")


# --- the forced-mode shapes of the older files

def test_ragged_shapes_route_512_rows_to_each_expert():
    """RAGGED of test_gpu_gemm_epilogue / test_gpu_gated / test_gpu_wscale /
    test_gpu_store16: E = 2, top-2, so every token selects both experts -
    512 rows each, full M tiles then empty ones, never a partly filled one."""
    from tests import (test_gpu_gated, test_gpu_gemm_epilogue,
                       test_gpu_store16, test_gpu_wscale)

    assert test_gpu_store16.RAGGED is test_gpu_gemm_epilogue.RAGGED
    assert test_gpu_store16.gated.RAGGED is test_gpu_gated.RAGGED
    for mod in (test_gpu_gemm_epilogue, test_gpu_gated, test_gpu_wscale):
        r = mod.RAGGED
        S, E, H = r["sequence_len"], r["num_experts"], r["hidden_size"]
        assert (S, E, r["expert_top_k"]) == (512, 2, 2)
        g = torch.Generator(device="cpu").manual_seed(47)
        x = torch.randn(1, S, H, generator=g).to(torch.bfloat16)
        gw = torch.randn(H, E, generator=g).to(torch.bfloat16)
        ocfg = OracleConfig(num_experts=E, expert_top_k=2, capacity_factor=2,
                            element="bf16")
        _, sel, _, _ = gate_forward(np32(x).reshape(S, H),
                                    np32(gw).reshape(E, H), ocfg)
        assert np.bincount(sel.reshape(-1), minlength=E).tolist() == [512, 512]
        assert expert_capacity(S, ocfg) == 1024
