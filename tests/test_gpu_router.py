"""Router variants on the GPU against tests/router_ref.py: sigmoid scoring,
a selection bias, group-limited top-k, unnormalised and scaled weights
(fm_router_config), through both gates.

Inputs, all from one Generator().manual_seed(47) in this order:
    x = randn(S, H); gw = randn(H, E) / sqrt(H); bias = 0.1 * randn(E);
    ew = randn(E + nSh, mats, P, H)
The 1/sqrt(H) keeps sigmoid scores off saturation. P = 256.

Shapes: capacity_factor is chosen so that the reference's largest load
fits EC (no schedule-dependent drops in the two-tile cases); R6 also runs
at CF 1 with drops, in one routing tile, where the kept set is
deterministic.

Bars are the project's own: bf16/fp16 rtol 2e-2, atol 2e-3 * scale; fp32
1e-5; MX the _assert_mx_values bar of tests/test_gpu_parity.py, restated
here. prob_sum against D: rtol 1e-5.

Near-tie escape: tokens whose margin (selection or group, in units of the
selection score c) is below 1e-4 are left out of the routing and value
comparisons; a case fails if more than 5 % of its tokens are left out.
"""
import ctypes
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle.moe_oracle import OracleConfig
from tests.router_ref import router_moe_forward
from tests.test_gpu_parity import (assert_values, fresh_moe,  # noqa: F401
                                   make_cfg, routing_from_lib)

pytestmark = pytest.mark.gpu

ELEMENT = {0: "fp32", 2: "bf16", 3: "fp16", 5: "bf16"}
FM_ERR_UNSUPPORTED = -4
ESCAPE = 1e-4
ROUTER_KEYS = ("scoring_func", "norm_topk_prob", "n_group", "topk_group",
               "group_score", "routed_scaling_factor")

V3 = dict(scoring_func=1, group_score=1, norm_topk_prob=1,
          routed_scaling_factor=2.5)
# name: (S, E, k, H, CF, router keys, bias?)
CASES = {
    "R1": (128, 8, 2, 128, 2,
           dict(norm_topk_prob=0, routed_scaling_factor=2.5), False),
    "R2": (256, 64, 6, 128, 4,
           dict(n_group=8, topk_group=3, group_score=0, norm_topk_prob=0,
                routed_scaling_factor=16.0), False),
    "R3": (256, 256, 8, 128, 16, dict(V3, n_group=8, topk_group=4), True),
    "R5": (256, 60, 4, 192, 2, dict(norm_topk_prob=0), False),
    "R6": (128, 8, 2, 128, 4, dict(scoring_func=1, norm_topk_prob=1), True),
    "R7": (256, 64, 8, 64, 8,
           dict(scoring_func=1, n_group=4, topk_group=2, group_score=1), True),
}


def case_cfg(name, **kw):
    S, E, k, H, CF, router, _ = CASES[name]
    base = dict(sequence_len=S, num_experts=E, expert_top_k=k, hidden_size=H,
                intermediate_size=256, capacity_factor=CF)
    base.update(router)
    base.update(kw)
    return make_cfg(**base)


def draw(cfg, seed=47):
    from flashmoe_amd.config import (expert_mats, num_shared, torch_dtype_of,
                                     weight_dtype_of)

    H, P, E = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_experts"]
    S = cfg["sequence_len"] * cfg["mini_batch"]
    dt = torch_dtype_of(cfg["torch_dtype"])
    wdt = weight_dtype_of(cfg["torch_dtype"])
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(S, H, generator=g)
    gw = torch.randn(H, E, generator=g) / H ** 0.5
    bias = 0.1 * torch.randn(E, generator=g)
    ew = torch.randn(E + num_shared(cfg), expert_mats(cfg["hidden_act"]), P, H,
                     generator=g)
    return (x.view(cfg["mini_batch"], cfg["sequence_len"], H).to(dt).cuda(),
            gw.to(dt).cuda(), bias.float().cuda(), ew.to(wdt).cuda())


_REF = {}


def reference(cfg, x, gw, bias, ew):
    """Computed once per (config, bias) and shared; never modified."""
    key = (json.dumps(cfg, sort_keys=True),
           None if bias is None else bias.cpu().numpy().tobytes())
    if key not in _REF:
        S = cfg["sequence_len"] * cfg["mini_batch"]
        ocfg = OracleConfig(
            num_experts=cfg["num_experts"], expert_top_k=cfg["expert_top_k"],
            capacity_factor=cfg["capacity_factor"],
            drop_tokens=cfg["drop_tokens"], hidden_act=cfg["hidden_act"],
            element=ELEMENT[cfg["torch_dtype"]],
            mx_fp8=(cfg["torch_dtype"] == 5))
        _REF[key] = router_moe_forward(
            x.view(S, -1).float().cpu().numpy(),
            gw.float().cpu().numpy().reshape(-1), ew.float().cpu().numpy(),
            ocfg, {k: cfg[k] for k in ROUTER_KEYS if k in cfg},
            None if bias is None else bias.cpu().numpy(),
            n_shared=cfg.get("num_shared_experts", 0))
    return _REF[key]


def ec_of(cfg):
    S = cfg["sequence_len"] * cfg["mini_batch"]
    base = -(-S // cfg["num_experts"]) if cfg["drop_tokens"] else S
    return base * cfg["capacity_factor"] * cfg["expert_top_k"]


def assert_mx_values(out, want):
    """tests/test_gpu_parity._assert_mx_values, restated."""
    got = out.float().cpu().numpy()
    scale = max(1.0, float(np.abs(want).max()))
    ok = np.isclose(got, want, rtol=5e-2, atol=5e-3 * scale)
    frac_bad = 1.0 - ok.mean()
    max_err = float(np.abs(got - want).max())
    assert frac_bad <= 1e-3 and max_err <= 0.025 * scale, (
        f"moe_out: {100*frac_bad:.4f}% outside tol, max err {max_err:.3f} "
        f"(scale {scale:.1f})")


def check_against_reference(cfg, ref, out, gate_out, what):
    """Counts, per-expert token lists, prob_sum, gate_out and moe_out."""
    S = cfg["sequence_len"] * cfg["mini_batch"]
    E, EC = cfg["num_experts"], ec_of(cfg)
    element = ELEMENT[cfg["torch_dtype"]]
    near = (ref["margin_sel"] < ESCAPE) | (ref["margin_grp"] < ESCAPE)
    print(f"{what}: {100.0 * near.mean():.2f}% of tokens inside the near-tie "
          f"escape; max load {int(ref['eC'].max())} / EC {EC}")
    assert near.mean() <= 0.05, f"{what}: {100 * near.mean():.2f}% left out"
    ok_tok = ~near
    counts, tok, ps = routing_from_lib(E, EC)
    if not near.any():
        assert np.array_equal(counts.astype(np.int64),
                              np.minimum(ref["eC"], EC)), f"{what}: counts"
    one_tile = S == 128
    for e in range(E):
        got = tok[e, : counts[e]].astype(np.int64)
        want = np.asarray(ref["token_lists"][e], dtype=np.int64)
        got_ps = ps[e, : counts[e]][ok_tok[got]]
        got, want = got[ok_tok[got]], want[ok_tok[want]]
        if not one_tile:
            order = np.argsort(got, kind="stable")
            got, got_ps, want = got[order], got_ps[order], np.sort(want)
        assert np.array_equal(got, want), f"{what}: expert {e} token list"
        assert np.allclose(got_ps, ref["D"][got], rtol=1e-5, atol=0), (
            f"{what}: expert {e} prob_sum, max rel err "
            f"{np.abs(got_ps / ref['D'][got] - 1).max():.2e}")
    bar = {} if element == "fp32" else dict(rtol=2e-2, atol_scale=2e-3)
    el = "fp32" if element == "fp32" else "bf16"
    assert_values(gate_out, ref["gate_out"], el, f"{what}: gate_out", **bar)
    rows = torch.from_numpy(np.nonzero(ok_tok)[0]).cuda()
    got_out = out.view(S, -1).index_select(0, rows)
    if cfg["torch_dtype"] == 5:
        assert_mx_values(got_out, ref["moe_out"][ok_tok])
    else:
        assert_values(got_out, ref["moe_out"][ok_tok], el,
                      f"{what}: moe_out", **bar)


@pytest.fixture
def gate_env():
    """FM_GATE_FUSED / FM_FUSED are re-read per forward; restore them."""
    saved = {k: os.environ.get(k) for k in ("FM_GATE_FUSED", "FM_FUSED")}
    yield os.environ
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def set_gate(env, gate):
    if gate == "two_kernel":
        env["FM_GATE_FUSED"] = "0"
    else:
        env.pop("FM_GATE_FUSED", None)


def run_case(moe, name, gate, env, **kw):
    set_gate(env, gate)
    cfg, path = case_cfg(name, **kw)
    moe.initialize(path, rank=0, world_size=1)
    x, gw, bias, ew = draw(cfg)
    if not CASES[name][6]:
        bias = None
    else:
        moe.set_score_bias(bias)
    got = moe.get_router()
    for k in ROUTER_KEYS:
        assert got[k] == pytest.approx(cfg.get(k, got[k]))
    assert (got["score_bias"] is None) == (bias is None)
    out = moe.moe_forward(x, gw, ew)
    gate_out = moe.gate_output().clone()
    torch.cuda.synchronize()
    import flashmoe_amd._ext as _ext

    assert _ext.load().fm_last_forward_fused() == 0
    ref = reference(cfg, x, gw, bias, ew)
    check_against_reference(cfg, ref, out, gate_out,
                            f"{name}/{gate}/dtype{cfg['torch_dtype']}")
    return cfg, ref


# --- parity, both gates

@pytest.mark.parametrize("gate", ["single_launch", "two_kernel"])
@pytest.mark.parametrize("name", ["R1", "R2", "R5", "R6", "R7"])
def test_variant_bf16(fresh_moe, gate_env, name, gate):
    cfg, ref = run_case(fresh_moe, name, gate, gate_env)
    assert int(ref["eC"].max()) <= ec_of(cfg), "case is meant not to overflow"


def test_v3_router_256_experts(fresh_moe, gate_env):
    """R3: E = 256 runs the two-kernel gate whatever the knob says."""
    cfg, ref = run_case(fresh_moe, "R3", "single_launch", gate_env)
    assert int(ref["eC"].max()) <= ec_of(cfg)
    # the limit binds: every token's 8 experts lie in at most 4 of 8 groups
    groups = ref["topk_idx"] // 32
    assert max(len(set(g)) for g in groups.tolist()) <= 4
    assert len({tuple(sorted(set(g))) for g in groups.tolist()}) > 8


@pytest.mark.parametrize("name", ["R2", "R6"])
def test_variant_fp32_valu_logits(fresh_moe, gate_env, name):
    run_case(fresh_moe, name, "single_launch", gate_env, torch_dtype=0)


def test_r6_capacity_one_deterministic_drops(fresh_moe, gate_env):
    """CF 1: EC = 32 against a largest load of 68, one routing tile: the
    kept set is the first 32 tokens of every expert, in order."""
    for gate in ("single_launch", "two_kernel"):
        cfg, ref = run_case(fresh_moe, "R6", gate, gate_env,
                            capacity_factor=1)
        assert ec_of(cfg) == 32 and int(ref["eC"].max()) > 32
        assert int((~ref["kept"]).sum()) > 0
        fresh_moe.finalize()


def test_r6_fp16(fresh_moe, gate_env):
    run_case(fresh_moe, "R6", "single_launch", gate_env, torch_dtype=3)


def test_r6_mx(fresh_moe, gate_env):
    run_case(fresh_moe, "R6", "single_launch", gate_env, torch_dtype=5)


def test_r7_swiglu_with_a_shared_expert(fresh_moe, gate_env):
    for gate in ("single_launch", "two_kernel"):
        run_case(fresh_moe, "R7", gate, gate_env, hidden_act=2,
                 num_shared_experts=1)
        fresh_moe.finalize()


# --- exact tests

def forward_raw(moe, cfg, x, gw, ew, out, stream=None):
    """fm_moe_forward on fixed pointers (out included); returns a clone of
    the output."""
    import flashmoe_amd._ext as _ext

    S = cfg["sequence_len"] * cfg["mini_batch"]
    out.zero_()
    torch.cuda.synchronize()
    st = stream.cuda_stream if stream is not None else \
        torch.cuda.current_stream().cuda_stream
    _ext.check(_ext.load().fm_moe_forward(
        ctypes.c_void_p(st), ctypes.c_void_p(x.data_ptr()),
        ctypes.c_void_p(gw.data_ptr()), ctypes.c_void_p(ew.data_ptr()),
        None, None, ctypes.c_void_p(moe.gate_output().data_ptr()),
        ctypes.c_void_p(out.data_ptr()), S), "fm_moe_forward")
    torch.cuda.synchronize()
    return out.clone()


@pytest.mark.parametrize("dtype_code", [2, 0])
@pytest.mark.parametrize("gate", ["single_launch", "two_kernel"])
def test_scaling_factor_two_doubles_the_output_exactly(fresh_moe, gate_env,
                                                       dtype_code, gate):
    """Every step commutes with an exact doubling: D = mCw / 2, the weight
    Element(s) / D, the Element rounding of the scaled row, the fp32 sum.
    One routing tile (S = 128) and H = 128 (two logits partials at most):
    both gates are deterministic here."""
    set_gate(gate_env, gate)
    outs = {}
    for factor in (None, 2.0):
        kw = {} if factor is None else dict(routed_scaling_factor=factor)
        cfg, path = make_cfg(capacity_factor=2, torch_dtype=dtype_code, **kw)
        fresh_moe.initialize(path, rank=0, world_size=1)
        x, gw, _, ew = draw(cfg)
        outs[factor] = fresh_moe.moe_forward(x, gw, ew).clone()
        torch.cuda.synchronize()
        fresh_moe.finalize()
    assert outs[None].float().abs().max() > 1.0
    assert torch.equal(outs[2.0], 2 * outs[None])


def test_explicit_defaults_equal_absent_keys(fresh_moe, gate_env):
    outs = []
    for kw in ({}, dict(scoring_func=0, norm_topk_prob=1, n_group=1,
                        topk_group=1, group_score=0,
                        routed_scaling_factor=1.0)):
        cfg, path = make_cfg(capacity_factor=2, **kw)
        fresh_moe.initialize(path, rank=0, world_size=1)
        x, gw, _, ew = draw(cfg)
        outs.append((fresh_moe.moe_forward(x, gw, ew).clone(),
                     fresh_moe.gate_output().clone()))
        torch.cuda.synchronize()
        fresh_moe.finalize()
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])


def test_graph_replay_bit_identical(fresh_moe, gate_env):
    """R7, five identical forwards on a side stream: eager, capture, three
    replays."""
    set_gate(gate_env, "single_launch")
    cfg, path = case_cfg("R7")
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, bias, ew = draw(cfg)
    fresh_moe.set_score_bias(bias)
    ref = reference(cfg, x, gw, bias, ew)
    out = torch.empty_like(x)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    outs = [forward_raw(fresh_moe, cfg, x, gw, ew, out, stream) for _ in range(5)]
    check_against_reference(cfg, ref, outs[-1], fresh_moe.gate_output(),
                            "R7 replay")
    for i, o in enumerate(outs):
        assert torch.equal(o, outs[0]), f"call {i} differs from call 0"


def test_router_change_after_capture(fresh_moe, gate_env):
    """fm_set_router between forwards on the same pointers: the captured
    graph of the old router must not be replayed."""
    import flashmoe_amd._ext as _ext

    set_gate(gate_env, "single_launch")
    lib = _ext.load()
    cfg, path = case_cfg("R1")
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, _, ew = draw(cfg)
    out = torch.empty_like(x)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    before = [forward_raw(fresh_moe, cfg, x, gw, ew, out, stream) for _ in range(3)]
    assert torch.equal(before[0], before[2])
    r = _ext.router_defaults()
    r.scoring_func, r.norm_topk_prob, r.routed_scaling_factor = 1, 1, 1.0
    _ext.check(lib.fm_set_router(ctypes.byref(r)), "fm_set_router")
    after = forward_raw(fresh_moe, cfg, x, gw, ew, out, stream)
    assert not torch.equal(after, before[0])
    # NULL = the defaults, again on the same pointers
    _ext.check(lib.fm_set_router(None), "fm_set_router")
    plain = forward_raw(fresh_moe, cfg, x, gw, ew, out, stream)
    assert not torch.equal(plain, after)
    fresh_moe.finalize()
    # fresh process-state runs of the two routers
    cfg2, path2 = case_cfg("R1", scoring_func=1, norm_topk_prob=1,
                           routed_scaling_factor=1.0)
    fresh_moe.initialize(path2, rank=0, world_size=1)
    assert fresh_moe.get_router()["scoring_func"] == 1
    assert torch.equal(forward_raw(fresh_moe, cfg2, x, gw, ew, out, stream), after)
    fresh_moe.finalize()
    cfg3, path3 = make_cfg(capacity_factor=2)
    fresh_moe.initialize(path3, rank=0, world_size=1)
    assert fresh_moe.get_router()["norm_topk_prob"] == 1  # reset by initialize
    assert torch.equal(forward_raw(fresh_moe, cfg3, x, gw, ew, out, stream), plain)


def test_bias_rewritten_in_place_between_replays(fresh_moe, gate_env):
    set_gate(gate_env, "single_launch")
    cfg, path = case_cfg("R6")
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, bias, ew = draw(cfg)
    bias = bias.clone()
    fresh_moe.set_score_bias(bias)
    out = torch.empty_like(x)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    ref0 = reference(cfg, x, gw, bias, ew)
    outs = [forward_raw(fresh_moe, cfg, x, gw, ew, out, stream) for _ in range(3)]
    check_against_reference(cfg, ref0, outs[2], fresh_moe.gate_output(),
                            "R6 first bias")
    new_bias = torch.zeros_like(bias)
    new_bias[5] = 1.0  # every token now selects expert 5 first
    bias.copy_(new_bias)
    torch.cuda.synchronize()
    again = forward_raw(fresh_moe, cfg, x, gw, ew, out, stream)  # a replay
    ref1 = reference(cfg, x, gw, bias, ew)
    assert (ref1["topk_idx"][:, 0] == 5).all()
    assert not np.array_equal(ref1["topk_idx"], ref0["topk_idx"])
    check_against_reference(cfg, ref1, again, fresh_moe.gate_output(),
                            "R6 rewritten bias")
    assert not torch.equal(again, outs[2])


# --- refusals and path

def _init_plain(moe, **kw):
    cfg, path = make_cfg(**kw)
    moe.initialize(path, rank=0, world_size=1)
    return cfg


@pytest.mark.parametrize("cfg_kw, router_kw, key", [
    ({}, dict(n_group=3, topk_group=1), "n_group"),
    ({}, dict(n_group=0), "n_group"),
    (dict(num_experts=64), dict(n_group=32, topk_group=32), "n_group"),
    ({}, dict(n_group=4, topk_group=5), "topk_group"),
    ({}, dict(n_group=4, topk_group=0), "topk_group"),
    ({}, dict(n_group=8, topk_group=1), "expert_top_k"),
    ({}, dict(n_group=8, topk_group=8, group_score=1), "group_score"),
    ({}, dict(routed_scaling_factor=0.0), "routed_scaling_factor"),
    ({}, dict(routed_scaling_factor=float("inf")), "routed_scaling_factor"),
    ({}, dict(routed_scaling_factor=float("nan")), "routed_scaling_factor"),
    (dict(expert_top_k=1), dict(norm_topk_prob=0), "norm_topk_prob"),
    (dict(expert_top_k=1), dict(routed_scaling_factor=2.0),
     "routed_scaling_factor"),
    (dict(is_training=1), dict(scoring_func=1), "scoring_func"),
    (dict(is_training=1), dict(norm_topk_prob=0), "norm_topk_prob"),
    (dict(num_experts=512), dict(scoring_func=1), "scoring_func"),
    (dict(num_experts=512), dict(n_group=8, topk_group=4), "n_group"),
])
def test_fm_set_router_refuses(fresh_moe, cfg_kw, router_kw, key):
    import flashmoe_amd._ext as _ext

    _init_plain(fresh_moe, **cfg_kw)
    lib = _ext.load()
    r = _ext.router_defaults()
    for k, v in router_kw.items():
        setattr(r, k, v)
    assert lib.fm_set_router(ctypes.byref(r)) == FM_ERR_UNSUPPORTED
    assert key.encode() in lib.fm_last_error()
    # the refused call left the default router in place
    got = fresh_moe.get_router()
    assert got["n_group"] == 1 and got["scoring_func"] == 0
    assert got["routed_scaling_factor"] == 1.0


def test_bias_refusals(fresh_moe):
    import flashmoe_amd._ext as _ext

    _init_plain(fresh_moe, num_experts=512)
    lib = _ext.load()
    b = torch.zeros(512, device="cuda")
    r = _ext.router_defaults()
    r.score_bias = b.data_ptr()
    assert lib.fm_set_router(ctypes.byref(r)) == FM_ERR_UNSUPPORTED
    assert b"score_bias" in lib.fm_last_error()
    with pytest.raises(ValueError, match="score bias"):
        fresh_moe.set_score_bias(b)
    # norm / factor alone work at E = 512
    r = _ext.router_defaults()
    r.norm_topk_prob, r.routed_scaling_factor = 0, 16.0
    assert lib.fm_set_router(ctypes.byref(r)) == 0
    fresh_moe.finalize()
    _init_plain(fresh_moe, is_training=1)
    with pytest.raises(RuntimeError, match="is_training"):
        fresh_moe.set_score_bias(torch.zeros(8, device="cuda"))
    for bad in (torch.zeros(8), torch.zeros(9, device="cuda"),
                torch.zeros(8, device="cuda", dtype=torch.float16)):
        with pytest.raises(ValueError, match="score bias"):
            fresh_moe.set_score_bias(bad)


def test_initialize_refuses_through_the_config(fresh_moe):
    for kw, key in ((dict(n_group=3), "n_group"),
                    (dict(expert_top_k=1, routed_scaling_factor=2.0),
                     "routed_scaling_factor")):
        _, path = make_cfg(**kw)
        with pytest.raises(ValueError, match=key):
            fresh_moe.initialize(path, rank=0, world_size=1)
        with pytest.raises(RuntimeError):
            fresh_moe.finalize()  # nothing was initialized


def test_norm_and_factor_at_512_experts(fresh_moe, gate_env):
    """The 64-token half-pass instantiation (E > 256, eight threads per
    token) under norm 0 / factor 16. The probabilities of 512 experts are
    small against the absolute escape: with H = 64 and top-2 the reference
    leaves out 3.12 % of the tokens."""
    cfg, path = make_cfg(sequence_len=128, num_experts=512, expert_top_k=2,
                         hidden_size=64, capacity_factor=8, norm_topk_prob=0,
                         routed_scaling_factor=16.0)
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, _, ew = draw(cfg)
    out = fresh_moe.moe_forward(x, gw, ew)
    gate_out = fresh_moe.gate_output().clone()
    torch.cuda.synchronize()
    ref = reference(cfg, x, gw, None, ew)
    assert int(ref["eC"].max()) <= ec_of(cfg)
    check_against_reference(cfg, ref, out, gate_out, "E512 norm0 x16")


def test_fused_request_runs_the_multi_kernel_path(fresh_moe, gate_env):
    """FM_FUSED=1: the default router takes the single-launch forward on
    this shape, a non-default one never does."""
    import flashmoe_amd._ext as _ext

    gate_env["FM_FUSED"] = "1"
    lib = _ext.load()
    cfg, path = make_cfg(sequence_len=256, capacity_factor=2)
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, _, ew = draw(cfg)
    fresh_moe.moe_forward(x, gw, ew)
    torch.cuda.synchronize()
    assert lib.fm_last_forward_fused() == 1  # the test is not vacuous
    fresh_moe.finalize()
    cfg, path = make_cfg(sequence_len=256, capacity_factor=2,
                         norm_topk_prob=0, routed_scaling_factor=2.5)
    fresh_moe.initialize(path, rank=0, world_size=1)
    out = fresh_moe.moe_forward(x, gw, ew)
    gate_out = fresh_moe.gate_output().clone()
    torch.cuda.synchronize()
    assert lib.fm_last_forward_fused() == 0
    check_against_reference(cfg, reference(cfg, x, gw, None, ew), out,
                            gate_out, "FM_FUSED=1 norm0 x2.5")


def test_staged_gate_forward_and_read_routing(fresh_moe, gate_env):
    """The EP building blocks under R2: fm_gate_forward + fm_read_routing."""
    import flashmoe_amd._ext as _ext

    cfg, path = case_cfg("R2")
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, _, ew = draw(cfg)
    S, E, EC = 256, cfg["num_experts"], ec_of(cfg)
    gate_out = fresh_moe.gate_output()
    _ext.check(_ext.load().fm_gate_forward(
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
        ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(gw.data_ptr()),
        ctypes.c_void_p(gate_out.data_ptr()), S), "fm_gate_forward")
    torch.cuda.synchronize()
    ref = reference(cfg, x, gw, None, ew)
    near = (ref["margin_sel"] < ESCAPE) | (ref["margin_grp"] < ESCAPE)
    assert near.mean() <= 0.05
    counts, tok, ps = routing_from_lib(E, EC)
    for e in range(E):
        got = tok[e, : counts[e]].astype(np.int64)
        keep = ~near[got]
        want = np.asarray(ref["token_lists"][e], dtype=np.int64)
        assert np.array_equal(np.sort(got[keep]), np.sort(want[~near[want]]))
        # norm 0, factor 16: every token's denominator is 1 / 16
        assert np.array_equal(ps[e, : counts[e]], np.full(counts[e], 1 / 16,
                                                          dtype=np.float32))
    assert_values(gate_out, ref["gate_out"], "bf16", "gate_out")
