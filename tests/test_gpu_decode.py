"""Decode-sized forwards (S = sequence_len * mini_batch in 1..127) on the GPU
(DESIGN.md par.5k): the masked gate tile, the weight-streaming expert FFN
(FM_DECODE_FFN=1) and the grouped GEMMs it is measured against
(FM_DECODE_FFN=0). The variable is re-read per forward, so every value case
runs under both by parametrisation.

References, unchanged: oracle.moe_oracle.moe_forward (plain experts),
tests/gated_ref.py (SwiGLU / GeGLU), tests/shared_ref.py (shared experts),
tests/router_ref.py (router variants).

Bars are the project's own (test_gpu_parity.assert_values): bf16, fp16 and
fp8-weights rtol 2e-2, atol 2e-3 * max(1, max|ref|), every element; fp32
1e-5; routing (counts and ordered token lists) bit-exact. S < 128 is one
routing tile, so the kept set is deterministic under drops.

Inputs are drawn x, gw, weights from Generator().manual_seed(47) as
test_gpu_parity.run_pair draws them; a case is used only if the oracle's
smallest tie_margin is at least 1e-3 (asserted). The router cases draw as
tests/test_gpu_router.py does (gw / sqrt(H), a bias) and carry that suite's
near-tie escape.
"""
import ctypes
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle.moe_oracle import OracleConfig, moe_forward as oracle_forward
from tests.gated_ref import gated_moe_forward
from tests.shared_ref import shared_moe_forward
from tests.test_gpu_parity import (assert_values, fresh_moe,  # noqa: F401
                                   make_cfg, routing_from_lib, run_pair)

pytestmark = pytest.mark.gpu

ELEMENT = {0: "fp32", 1: "fp32", 2: "bf16", 3: "fp16", 4: "bf16"}
FM_ERR_SHAPE = -3
FM_ERR_UNSUPPORTED = -4
MIN_TIE_MARGIN = 1e-3
FFN = ["1", "0"]  # FM_DECODE_FFN: the streaming kernels / the grouped GEMMs

# defaults: H = 128, P = 256, bf16, E = 8, top-2, capacity_factor 1, drop
CASES = {
    1: dict(S=1),
    2: dict(S=1, expert_top_k=8),
    3: dict(S=7),
    4: dict(S=16),
    5: dict(S=17),
    6: dict(S=64),
    7: dict(S=127),
    8: dict(S=127, num_experts=2, expert_top_k=2, drop_tokens=0),
    9: dict(S=33, num_experts=4, expert_top_k=1),
    10: dict(S=100, num_experts=4, expert_top_k=1, drop_tokens=0),
    11: dict(S=4, num_experts=256, expert_top_k=8),
    12: dict(S=64, num_experts=256, expert_top_k=8),
    13: dict(S=96, num_experts=64, expert_top_k=6, capacity_factor=2),
    14: dict(S=17, hidden_size=192, intermediate_size=320),
}
ROUTING_CASES = (1, 3, 6, 9, 11, 12)

# The shapes above keep K = H or P at 128..320, so a wave of k_decode_ffn
# (four waves interleave 128-element K chunks) sees one chunk at most. These
# run its steady-state loop: H = 1024 is 8 chunks (two per wave), P = 1600 is
# 12.5 (three or four per wave, both register sets, the restaging of the
# wave's A region, and a ragged 64-element last chunk that is not a wave's
# first). S = 8: EC = 2; S = 40: EC = 10, one fragment, drops.
LONG_K = dict(hidden_size=1024, intermediate_size=1600)


def case_kw(n, **kw):
    """make_cfg keywords of a table case: the natural decode config,
    sequence_len 1 and mini_batch S."""
    c = dict(CASES[n])
    c.update(kw)
    S = c.pop("S")
    return dict(sequence_len=1, mini_batch=S, **c)


def bar(element):
    # assert_values applies its fp32 bar to everything that is not "bf16";
    # fp16 carries the bf16 bar (as in test_gpu_gated)
    return {} if element == "fp32" else dict(rtol=2e-2, atol_scale=2e-3)


def ec_of(cfg):
    S = cfg["sequence_len"] * cfg["mini_batch"]
    base = -(-S // cfg["num_experts"]) if cfg["drop_tokens"] else S
    return base * cfg["capacity_factor"] * cfg["expert_top_k"]


def draw(cfg, seed=47):
    """run_pair's draw, with the slab count of the config (a third slab for
    gated experts, the shared experts' slabs last)."""
    from flashmoe_amd.config import (expert_mats, num_shared, torch_dtype_of,
                                     weight_dtype_of)

    H, P, E = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_experts"]
    dt = torch_dtype_of(cfg["torch_dtype"])
    wdt = weight_dtype_of(cfg["torch_dtype"])
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(cfg["mini_batch"], cfg["sequence_len"], H,
                    generator=g).to(dt).cuda()
    gw = torch.randn(H, E, generator=g).to(dt).cuda()
    ew = torch.randn(E + num_shared(cfg), expert_mats(cfg["hidden_act"]), P, H,
                     generator=g).to(wdt).cuda()
    return x, gw, ew


_REF = {}


def reference(cfg, x, gw, ew, b_up=None, b_dn=None):
    """Computed once per config and shared between the FM_DECODE_FFN arms;
    never modified."""
    key = (json.dumps(cfg, sort_keys=True), b_up is not None, b_dn is not None)
    if key in _REF:
        return _REF[key]
    S = cfg["sequence_len"] * cfg["mini_batch"]
    nSh = cfg.get("num_shared_experts", 0)
    ocfg = OracleConfig(
        num_experts=cfg["num_experts"], expert_top_k=cfg["expert_top_k"],
        capacity_factor=cfg["capacity_factor"], drop_tokens=cfg["drop_tokens"],
        hidden_act=cfg["hidden_act"], element=ELEMENT[cfg["torch_dtype"]])
    xs = x.reshape(S, -1).float().cpu().numpy()
    gws = gw.float().cpu().numpy().reshape(-1)
    ews = ew.float().cpu().numpy()
    bu = b_up.float().cpu().numpy() if b_up is not None else None
    bd = b_dn.float().cpu().numpy() if b_dn is not None else None
    if nSh > 0 or (cfg["hidden_act"] >= 2 and bd is not None):
        assert bu is None
        ref = shared_moe_forward(xs, gws, ews, ocfg, nSh, bd)
    elif cfg["hidden_act"] >= 2:
        ref = gated_moe_forward(xs, gws, ews, ocfg)
    else:
        ref = oracle_forward(xs, gws, ews, ocfg, b_up=bu, b_dn=bd)
    margin = float(ref["tie_margin"].min())
    print(f"S={S} E={cfg['num_experts']} k={cfg['expert_top_k']}: min "
          f"tie_margin {margin:.2e}, max load {int(ref['eC'].max())} / EC "
          f"{ec_of(cfg)}, {int((ref['eC'] == 0).sum())} empty experts, "
          f"{int((~ref['kept']).sum())} dropped slots")
    assert margin >= MIN_TIE_MARGIN, "case too close to a routing tie"
    _REF[key] = ref
    return ref


@pytest.fixture
def env():
    """The knobs are re-read per forward; restore them."""
    keys = ("FM_DECODE_FFN", "FM_GATE_FUSED", "FM_FUSED")
    saved = {k: os.environ.get(k) for k in keys}
    yield os.environ
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def check_routing(cfg, ref):
    E, EC = cfg["num_experts"], ec_of(cfg)
    counts, tok, ps = routing_from_lib(E, EC)
    assert np.array_equal(counts.astype(np.int64), np.minimum(ref["eC"], EC))
    for e in range(E):
        assert np.array_equal(tok[e, : counts[e]].astype(np.int64),
                              ref["token_lists"][e]), f"expert {e} token list"
        if cfg["expert_top_k"] > 1:
            assert np.allclose(ps[e, : counts[e]],
                               ref["mCw"][tok[e, : counts[e]]], rtol=1e-3)


def check_values(cfg, out, gate_out, ref, what="moe_out"):
    S = cfg["sequence_len"] * cfg["mini_batch"]
    element = ELEMENT[cfg["torch_dtype"]]
    assert tuple(out.shape[-1:]) == (cfg["hidden_size"],)
    if gate_out is not None:
        assert gate_out.shape[0] == S
        assert_values(gate_out, ref["gate_out"], element, "gate_out",
                      **bar(element))
    assert_values(out.reshape(S, -1), ref["moe_out"], element, what,
                  **bar(element))


# unset FM_DECODE_FFN: (S, torch_dtype, takes the streaming kernels)
DEFAULT_ARM = [(4, 2, True), (5, 2, False), (16, 4, True), (17, 4, False),
               (8, 3, True), (9, 3, False),
               (4, 0, False), (64, 2, False)]


def run_decode(moe, env, ffn, routing=False, gate=True, **kw):
    env["FM_DECODE_FFN"] = ffn
    cfg, path = make_cfg(**kw)
    moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    out = moe.moe_forward(x, gw, ew)
    gate_out = moe.gate_output().clone()
    torch.cuda.synchronize()
    import flashmoe_amd._ext as _ext

    assert _ext.load().fm_last_forward_fused() == 0
    ref = reference(cfg, x, gw, ew)
    if routing:
        check_routing(cfg, ref)
    check_values(cfg, out, gate_out if gate else None, ref)
    return cfg, out, ref


# --- the table: bf16, relu

@pytest.mark.parametrize("ffn", FFN)
@pytest.mark.parametrize("n", sorted(CASES))
def test_case(fresh_moe, env, n, ffn):
    routing = n in ROUTING_CASES
    cfg, out, ref = run_decode(fresh_moe, env, ffn, routing=routing,
                               gate=routing, **case_kw(n))
    S = cfg["sequence_len"] * cfg["mini_batch"]
    got = out.reshape(S, -1).float().cpu().numpy()
    gone = ~ref["kept"].any(axis=1)
    empty = int((ref["eC"] == 0).sum())
    dropped = int((~ref["kept"]).sum())
    # the oracle facts the shapes were chosen for
    facts = {1: empty == 6, 2: empty == 0, 3: dropped == 4 and empty == 1,
             4: dropped == 7 and int(gone.sum()) == 1,
             5: int(ref["eC"].max()) <= 16,
             6: dropped == 13 and int(gone.sum()) == 4,
             8: list(ref["eC"]) == [127, 127],
             7: ec_of(cfg) == 32 and 16 < int(ref["eC"].max()),
             9: int(gone.sum()) == 3, 10: dropped == 0,
             11: empty == 225, 12: empty == 40 and dropped == 1,
             13: dropped == 0, 14: int(ref["eC"].max()) <= 16}
    assert facts.get(n, True), f"case {n} no longer has the shape it was for"
    # a token with every slot dropped: its row is exactly zero
    assert not got[gone].any()


@pytest.mark.parametrize("ffn", FFN)
@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("dtype_code", [2, 4])
@pytest.mark.parametrize("S", [8, 40])
def test_long_k(fresh_moe, env, S, dtype_code, act, ffn):
    """Several K chunks per wave, the last one ragged (see LONG_K)."""
    import flashmoe_amd._ext as _ext

    run_decode(fresh_moe, env, ffn, routing=True, sequence_len=1,
               mini_batch=S, torch_dtype=dtype_code, hidden_act=act, **LONG_K)
    assert _ext.load().fm_last_forward_decode_ffn() == int(ffn)


@pytest.mark.parametrize("S,dtype_code,streaming", DEFAULT_ARM)
def test_unset_knob_takes_the_measured_default(fresh_moe, env, S, dtype_code,
                                               streaming):
    """Both sides of the default's thresholds: which arm
    ran, from fm_last_forward_decode_ffn, and the values. Replays of the
    captured graph keep the answer."""
    import flashmoe_amd._ext as _ext

    cfg, path = make_cfg(sequence_len=1, mini_batch=S, torch_dtype=dtype_code,
                         hidden_act=2)
    env.pop("FM_DECODE_FFN", None)
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    for _ in range(3):
        out = fresh_moe.moe_forward(x, gw, ew)
        gate_out = fresh_moe.gate_output().clone()
        torch.cuda.synchronize()
        assert _ext.load().fm_last_forward_decode_ffn() == int(streaming)
    check_values(cfg, out, gate_out, reference(cfg, x, gw, ew))


# --- dtypes: fp16, fp8 weights, fp32 (fp32 takes the fp32 GEMM either way)

@pytest.mark.parametrize("ffn", FFN)
@pytest.mark.parametrize("dtype_code", [3, 4, 0])
@pytest.mark.parametrize("n", [6, 8])
def test_dtypes(fresh_moe, env, n, dtype_code, ffn):
    run_decode(fresh_moe, env, ffn, **case_kw(n, torch_dtype=dtype_code))


# --- activations: gelu, SwiGLU, GeGLU ([E, 3, P, H] when gated)

@pytest.mark.parametrize("ffn", FFN)
@pytest.mark.parametrize("act", [1, 2, 3])
@pytest.mark.parametrize("n", [3, 6, 8, 14])
def test_activations(fresh_moe, env, n, act, ffn):
    run_decode(fresh_moe, env, ffn, **case_kw(n, hidden_act=act))


def forward_raw(moe, cfg, x, gw, ew, gate_out, out, b_up=None, b_dn=None,
                stream=None):
    import flashmoe_amd._ext as _ext

    S = cfg["sequence_len"] * cfg["mini_batch"]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = stream.cuda_stream if stream is not None else \
        torch.cuda.current_stream().cuda_stream
    _ext.check(_ext.load().fm_moe_forward(
        ctypes.c_void_p(st), ptr(x), ptr(gw), ptr(ew), ptr(b_up), ptr(b_dn),
        ptr(gate_out), ptr(out), S), "fm_moe_forward")
    torch.cuda.synchronize()


@pytest.mark.parametrize("ffn", FFN)
@pytest.mark.parametrize("act,with_up", [(0, True), (2, False)])
def test_biases_through_the_abi(fresh_moe, env, act, with_up, ffn):
    """Case 6 with b_up + b_dn (relu) and with b_dn alone (SwiGLU)."""
    env["FM_DECODE_FFN"] = ffn
    cfg, path = make_cfg(**case_kw(6, hidden_act=act))
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    E, H, P = cfg["num_experts"], cfg["hidden_size"], cfg["intermediate_size"]
    g = torch.Generator().manual_seed(321)
    b_up = torch.randn(E, P, generator=g).to(x.dtype).cuda() if with_up else None
    b_dn = torch.randn(E, H, generator=g).to(x.dtype).cuda()
    out = torch.empty(64, H, dtype=x.dtype, device="cuda")
    forward_raw(fresh_moe, cfg, x, gw, ew, fresh_moe.gate_output(), out,
                b_up, b_dn)
    ref = reference(cfg, x, gw, ew, b_up, b_dn)
    check_values(cfg, out, fresh_moe.gate_output(), ref, "moe_out(bias)")


# --- shared experts (SwiGLU)

@pytest.mark.parametrize("ffn", FFN)
@pytest.mark.parametrize("nsh", [1, 2])
@pytest.mark.parametrize("n", [4, 9])
def test_shared_experts(fresh_moe, env, n, nsh, ffn):
    cfg, out, ref = run_decode(
        fresh_moe, env, ffn, **case_kw(n, hidden_act=2,
                                       num_shared_experts=nsh))
    S = cfg["sequence_len"] * cfg["mini_batch"]
    gone = ~ref["kept"].any(axis=1)
    assert int(gone.sum()) == {4: 1, 9: 3}[n]
    # the wholly dropped tokens carry exactly their shared sum
    el = ELEMENT[cfg["torch_dtype"]]
    from oracle.moe_oracle import _elem_round

    assert np.array_equal(ref["moe_out"][gone],
                          _elem_round(ref["shared_out"][gone], el))
    got = out.reshape(S, -1).float().cpu().numpy()
    assert np.abs(got[gone]).max() > 1.0
    assert_values(out.reshape(S, -1)[torch.from_numpy(gone).cuda()],
                  _elem_round(ref["shared_out"][gone], el), el,
                  "shared term of the dropped tokens")


# --- router variants (tests/router_ref.py, drawn as tests/test_gpu_router.py)

@pytest.mark.parametrize("ffn", FFN)
@pytest.mark.parametrize("which", ["v3_case12", "no_norm_case6"])
def test_router_variants(fresh_moe, env, which, ffn):
    from tests.test_gpu_router import (check_against_reference,
                                       draw as router_draw,
                                       reference as router_reference)

    env["FM_DECODE_FFN"] = ffn
    if which == "v3_case12":
        kw = case_kw(12, scoring_func=1, group_score=1, norm_topk_prob=1,
                     routed_scaling_factor=2.5, n_group=8, topk_group=4)
    else:
        kw = case_kw(6, norm_topk_prob=0)
    cfg, path = make_cfg(**kw)
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, bias, ew = router_draw(cfg)
    if which == "v3_case12":
        fresh_moe.set_score_bias(bias)
    else:
        bias = None
    out = fresh_moe.moe_forward(x, gw, ew)
    gate_out = fresh_moe.gate_output().clone()
    torch.cuda.synchronize()
    ref = router_reference(cfg, x, gw, bias, ew)
    check_against_reference(cfg, ref, out, gate_out, f"{which}/ffn{ffn}")


# --- buffers: exactly S rows are read and written

@pytest.mark.parametrize("ffn", FFN)
@pytest.mark.parametrize("top_k", [2, 1])
def test_rows_past_s_are_untouched(fresh_moe, env, top_k, ffn):
    """S = 17 through the raw ABI. gate_out and moe_out are the first 17
    rows of larger sentinel-filled buffers; x is followed by rows of NaN."""
    env["FM_DECODE_FFN"] = ffn
    cfg, path = make_cfg(**case_kw(5, expert_top_k=top_k))
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    S, H, PX, ROWS = 17, cfg["hidden_size"], 64, 160
    xbig = torch.full((ROWS, H), float("nan"), dtype=x.dtype, device="cuda")
    xbig[:S] = x.view(S, H)
    SENT = 0x5A5A
    gbig = torch.full((ROWS, PX), SENT, dtype=torch.int16, device="cuda")
    obig = torch.full((ROWS, H), SENT, dtype=torch.int16, device="cuda")
    forward_raw(fresh_moe, cfg, xbig, gw, ew, gbig.view(x.dtype),
                obig.view(x.dtype))
    assert bool((gbig[S:] == SENT).all()), "gate_out written past row S"
    assert bool((obig[S:] == SENT).all()), "moe_out written past row S"
    ref = reference(cfg, x, gw, ew)
    check_routing(cfg, ref)
    check_values(cfg, obig.view(x.dtype)[:S], gbig.view(x.dtype)[:S], ref)


# --- reproducibility

def test_five_forwards_bit_identical(fresh_moe, env):
    """Case 12 on a side stream: eager, the internal capture, three replays,
    under the streaming kernels."""
    env["FM_DECODE_FFN"] = "1"
    cfg, path = make_cfg(**case_kw(12))
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    out = torch.empty(64, cfg["hidden_size"], dtype=x.dtype, device="cuda")
    gate_out = fresh_moe.gate_output()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    outs, gates = [], []
    for _ in range(5):
        out.zero_()
        gate_out.zero_()
        torch.cuda.synchronize()
        forward_raw(fresh_moe, cfg, x, gw, ew, gate_out, out, stream=stream)
        outs.append(out.clone())
        gates.append(gate_out.clone())
    check_values(cfg, outs[-1], gates[-1], reference(cfg, x, gw, ew))
    for i in range(1, 5):
        assert torch.equal(outs[i], outs[0]), f"moe_out of call {i} differs"
        assert torch.equal(gates[i], gates[0]), f"gate_out of call {i} differs"


# --- path

@pytest.mark.parametrize("ffn", FFN)
@pytest.mark.parametrize("knob", ["FM_FUSED", "FM_GATE_FUSED"])
def test_single_launch_kernels_are_never_taken(fresh_moe, env, knob, ffn):
    """S = 64: asking for k_moe_fused / k_gate_fused changes nothing."""
    import flashmoe_amd._ext as _ext

    env[knob] = "1"
    cfg, out, ref = run_decode(fresh_moe, env, ffn, routing=True,
                               **case_kw(6))
    assert _ext.load().fm_last_forward_fused() == 0


# --- refusals through the C-ABI

def _raw_init(**kw):
    import flashmoe_amd._ext as _ext

    world = kw.pop("world_size", 1)
    base = dict(num_experts=8, expert_top_k=2, capacity_factor=1,
                drop_tokens=1, hidden_act=0, hidden_size=128,
                intermediate_size=256, sequence_len=1, mini_batch=64,
                dtype=2, is_training=0, num_shared_experts=0)
    base.update(kw)
    lib = _ext.load()
    c = _ext.FMConfig(**base)
    rc = lib.fm_initialize(ctypes.byref(c), 0, world)
    msg = lib.fm_last_error().decode()
    if rc == 0:
        lib.fm_finalize()
    return rc, msg


@pytest.mark.parametrize("kw,key", [
    (dict(dtype=5), "torch_dtype"),
    (dict(is_training=1), "is_training"),
    (dict(world_size=2), "world_size"),
])
def test_initialize_refuses_at_decode_sizes(kw, key):
    rc, msg = _raw_init(**kw)
    assert rc == FM_ERR_UNSUPPORTED, msg
    assert key in msg and "64" in msg, msg
    # the same config at 128 tokens initializes
    rc, msg = _raw_init(mini_batch=128, **kw)
    assert rc == 0, msg


def test_initialize_refuses_a_ragged_tail_behind_full_tiles():
    rc, msg = _raw_init(mini_batch=200)
    assert rc == FM_ERR_SHAPE, msg
    assert "200" in msg, msg


def test_initialize_accepts_every_decode_size():
    for S in (1, 2, 63, 127):
        rc, msg = _raw_init(mini_batch=S)
        assert rc == 0, (S, msg)


# --- no change at 128 tokens and above

def test_the_knob_is_inert_at_128(fresh_moe, env):
    outs = []
    for ffn in FFN:
        env["FM_DECODE_FFN"] = ffn
        cfg, path = make_cfg()
        out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
        outs.append((out.clone(), gate_out.clone()))
        fresh_moe.finalize()
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
