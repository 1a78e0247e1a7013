"""Per-output-channel weight scales of fp8 expert weights (torch_dtype 4 and
5, fm_set_weight_scales) on the GPU against tests/wscale_ref.py.

Scales are exp2(U(-2, 1)) drawn per (expert, slot, channel) from
Generator().manual_seed(48): swapped experts, swapped slots, glu / up
confusion and column offsets all show. Inputs are drawn as in
test_gpu_gated.draw with seed 47. The reference scales the fp32 matmul result
where the kernels do, so the bars are the project's own with every element
inside: bf16 rtol 2e-2, atol 2e-3 * max(1, max|ref|); dtype 5 the existing MX
bars. At the default shape the UNSCALED forward lies outside the bf16 bar on
93 % of the elements (relu and SwiGLU, checked on the CPU), so a kernel that
ignores or misindexes the scales fails.

capacity_factor 2 wherever S > 128: nothing is dropped. FM_FORCE_MODE,
FM_PERSIST_BLOCKS and FM_FUSED cases each run in one fresh child process.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle.moe_oracle import OracleConfig
from tests.conftest import REPO_ROOT
from tests.test_gpu_parity import (_assert_mx_values, assert_values,  # noqa: F401
                                   fresh_moe, make_cfg)
from tests.wscale_ref import wscale_expert_ffn, wscale_moe_forward

pytestmark = pytest.mark.gpu

FM_ERR_UNSUPPORTED = -4
BF16_BAR = dict(rtol=2e-2, atol_scale=2e-3)
MX_SMALL_BAR = dict(rtol=5e-2, atol_scale=5e-3)


def n_records(cfg):
    return cfg["num_experts"] + cfg.get("num_shared_experts", 0)


def record_len(cfg):
    P, H = cfg["intermediate_size"], cfg["hidden_size"]
    return P + H + (P if cfg["hidden_act"] >= 2 else 0)


def draw(cfg, seed=47):
    """test_gpu_gated.draw with E + nSh expert slabs (shared ones last)."""
    from flashmoe_amd.config import (expert_mats, torch_dtype_of,
                                     weight_dtype_of)

    H, P = cfg["hidden_size"], cfg["intermediate_size"]
    dt = torch_dtype_of(cfg["torch_dtype"])
    wdt = weight_dtype_of(cfg["torch_dtype"])
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(cfg["mini_batch"], cfg["sequence_len"], H,
                    generator=g).to(dt).cuda()
    gw = torch.randn(H, cfg["num_experts"], generator=g).to(dt).cuda()
    ew = torch.randn(n_records(cfg), expert_mats(cfg["hidden_act"]), P, H,
                     generator=g).to(wdt).cuda()
    return x, gw, ew


def draw_scales(cfg, seed=48):
    g = torch.Generator(device="cpu").manual_seed(seed)
    u = torch.rand(n_records(cfg), record_len(cfg), generator=g)
    return torch.exp2(3.0 * u - 2.0).cuda()


def oracle_cfg(cfg):
    return OracleConfig(
        num_experts=cfg["num_experts"], expert_top_k=cfg["expert_top_k"],
        capacity_factor=cfg["capacity_factor"], drop_tokens=cfg["drop_tokens"],
        hidden_act=cfg["hidden_act"], element="bf16",
        mx_fp8=(cfg["torch_dtype"] == 5))


_REF = {}


def reference(cfg, x, gw, ew, sc, b_up=None, b_dn=None, tag="seed48"):
    """Computed once per (config, scale values) and shared; never modified."""
    key = (json.dumps(cfg, sort_keys=True), tag, b_up is not None,
           b_dn is not None)
    if key not in _REF:
        S = cfg["sequence_len"] * cfg["mini_batch"]
        ref = wscale_moe_forward(
            x.reshape(S, -1).float().cpu().numpy(),
            gw.float().cpu().numpy().reshape(-1), ew.float().cpu().numpy(),
            oracle_cfg(cfg), sc.cpu().numpy(),
            cfg.get("num_shared_experts", 0),
            b_up.float().cpu().numpy() if b_up is not None else None,
            b_dn.float().cpu().numpy() if b_dn is not None else None)
        if S > 128:  # none dropped: the kept set is deterministic
            assert int(ref["eC"].sum()) == S * cfg["expert_top_k"]
        _REF[key] = ref
    return _REF[key]


def check(cfg, out, ref, what="moe_out", bar=None):
    S = cfg["sequence_len"] * cfg["mini_batch"]
    assert_values(out.reshape(S, -1), ref["moe_out"], "bf16", what,
                  **(bar or BF16_BAR))


def run_scaled(moe, bar=None, **kw):
    kw.setdefault("torch_dtype", 4)
    cfg, path = make_cfg(**kw)
    moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    sc = draw_scales(cfg)
    moe.set_weight_scales(sc)
    assert moe.get_weight_scales() is sc
    out = moe.moe_forward(x, gw, ew)
    torch.cuda.synchronize()
    check(cfg, out, reference(cfg, x, gw, ew, sc), bar=bar)
    return cfg, out


# --- dtype 4 parity, in-process (the synchronous 128x128 tile)

@pytest.mark.parametrize("act", [0, 2])
def test_default_shape(fresh_moe, act):
    run_scaled(fresh_moe, hidden_act=act)


def test_geglu(fresh_moe):
    run_scaled(fresh_moe, hidden_act=3)


@pytest.mark.parametrize("act", [0, 2])
def test_top1_direct_store(fresh_moe, act):
    run_scaled(fresh_moe, hidden_act=act, expert_top_k=1)


def test_ragged_columns_swiglu(fresh_moe):
    """H = 192 / P = 320: the column guards and the scale index both act."""
    run_scaled(fresh_moe, hidden_act=2, hidden_size=192, intermediate_size=320,
               sequence_len=256, capacity_factor=2)


def test_shared_expert_swiglu(fresh_moe):
    """The shared expert's record is the last one."""
    run_scaled(fresh_moe, hidden_act=2, num_shared_experts=1)


def forward_raw(moe, cfg, x, gw, ew, b_up=None, b_dn=None, out=None,
                stream=None):
    """fm_moe_forward through the raw ABI, into `out` (a fresh tensor by
    default) on `stream` (torch's current stream by default)."""
    import flashmoe_amd._ext as _ext

    S = cfg["sequence_len"] * cfg["mini_batch"]
    if out is None:
        out = torch.empty(S, cfg["hidden_size"], dtype=torch.bfloat16,
                          device="cuda")
    st = (stream or torch.cuda.current_stream()).cuda_stream
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    _ext.check(_ext.load().fm_moe_forward(
        ctypes.c_void_p(st), ptr(x), ptr(gw), ptr(ew), ptr(b_up), ptr(b_dn),
        ptr(moe.gate_output()), ptr(out), S), "fm_moe_forward")
    torch.cuda.synchronize()
    return out


def draw_biases(cfg, seed=321):
    g = torch.Generator(device="cpu").manual_seed(seed)
    b_up = torch.randn(n_records(cfg), cfg["intermediate_size"],
                       generator=g).to(torch.bfloat16).cuda()
    b_dn = torch.randn(n_records(cfg), cfg["hidden_size"],
                       generator=g).to(torch.bfloat16).cuda()
    return b_up, b_dn


def test_gelu_with_biases_scale_then_bias(fresh_moe):
    """act(acc * s_up + b_up) and acc * s_dn + b_dn through the raw ABI."""
    cfg, path = make_cfg(torch_dtype=4, hidden_act=1)
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    sc = draw_scales(cfg)
    b_up, b_dn = draw_biases(cfg)
    fresh_moe.set_weight_scales(sc)
    out = forward_raw(fresh_moe, cfg, x, gw, ew, b_up, b_dn)
    check(cfg, out, reference(cfg, x, gw, ew, sc, b_up, b_dn))


# --- decode-sized forwards

@pytest.fixture
def env():
    """FM_DECODE_FFN is re-read per forward; restore it."""
    saved = os.environ.get("FM_DECODE_FFN")
    os.environ.pop("FM_DECODE_FFN", None)
    yield os.environ
    if saved is None:
        os.environ.pop("FM_DECODE_FFN", None)
    else:
        os.environ["FM_DECODE_FFN"] = saved


@pytest.mark.parametrize("ffn", [None, "0"])
@pytest.mark.parametrize("act", [0, 2])
def test_decode_s4(fresh_moe, env, act, ffn):
    """S = 4: the default takes k_decode_ffn, FM_DECODE_FFN=0 the grouped
    GEMMs."""
    import flashmoe_amd._ext as _ext

    if ffn is not None:
        env["FM_DECODE_FFN"] = ffn
    run_scaled(fresh_moe, hidden_act=act, sequence_len=1, mini_batch=4)
    assert _ext.load().fm_last_forward_decode_ffn() == (1 if ffn is None else 0)


@pytest.mark.parametrize("act", [0, 2])
def test_decode_several_row_passes(fresh_moe, env, act):
    """S = 96, E = 2, top-2, no drop: each expert has 96 rows, three passes
    of k_decode_ffn."""
    import flashmoe_amd._ext as _ext

    env["FM_DECODE_FFN"] = "1"
    run_scaled(fresh_moe, hidden_act=act, sequence_len=1, mini_batch=96,
               num_experts=2, drop_tokens=0)
    assert _ext.load().fm_last_forward_decode_ffn() == 1


# --- EP entry points through the raw ABI (SwiGLU: three vectors per record)

def _ffn_setup(moe, seed):
    cfg, path = make_cfg(torch_dtype=4, hidden_act=2)
    moe.initialize(path, rank=0, world_size=1)
    g = torch.Generator().manual_seed(seed)
    ew = torch.randn(cfg["num_experts"], 3, cfg["intermediate_size"],
                     cfg["hidden_size"], generator=g).to(
                         torch.float8_e4m3fn).cuda()
    sc = draw_scales(cfg)
    moe.set_weight_scales(sc)
    return cfg, g, ew, sc


def _ffn_want(cfg, rows, ew, sc, e):
    return wscale_expert_ffn(rows.float().cpu().numpy(),
                             ew[e].float().cpu().numpy(),
                             sc[e].cpu().numpy(), oracle_cfg(cfg))


def test_expert_ffn_local_expert_3(fresh_moe):
    """A wrong scale stride or base reads another expert's record."""
    import flashmoe_amd._ext as _ext

    cfg, g, ew, sc = _ffn_setup(fresh_moe, 99)
    rows = torch.randn(64, cfg["hidden_size"], generator=g).to(
        torch.bfloat16).cuda()
    out = torch.empty_like(rows)
    st = torch.cuda.current_stream().cuda_stream
    _ext.check(_ext.load().fm_expert_ffn(
        ctypes.c_void_p(st), ctypes.c_void_p(rows.data_ptr()),
        ctypes.c_void_p(ew.data_ptr()), None, None,
        ctypes.c_void_p(out.data_ptr()), 64, 3), "fm_expert_ffn")
    torch.cuda.synchronize()
    assert_values(out, _ffn_want(cfg, rows, ew, sc, 3), "bf16", "expert_ffn",
                  **BF16_BAR)


def test_expert_ffn_segments_mapped(fresh_moe):
    """Two [EC, H] segments mapped to experts 5, 1: the scales follow the
    weight expert, not the segment index."""
    import flashmoe_amd._ext as _ext

    cfg, g, ew, sc = _ffn_setup(fresh_moe, 101)
    H, EC = cfg["hidden_size"], 32  # EC = ceil(128/8) * CF 1 * top-2
    rows = torch.randn(2, EC, H, generator=g).to(torch.bfloat16).cuda()
    seg = torch.tensor([5, 1], dtype=torch.int32, device="cuda")
    out = torch.empty_like(rows)
    st = torch.cuda.current_stream().cuda_stream
    _ext.check(_ext.load().fm_expert_ffn_segments(
        ctypes.c_void_p(st), ctypes.c_void_p(rows.data_ptr()),
        ctypes.c_void_p(seg.data_ptr()), 2, ctypes.c_void_p(ew.data_ptr()),
        ctypes.c_void_p(out.data_ptr())), "fm_expert_ffn_segments")
    torch.cuda.synchronize()
    for s, e in enumerate((5, 1)):
        assert_values(out[s], _ffn_want(cfg, rows[s], ew, sc, e), "bf16",
                      f"ffn_segments[seg {s}]", **BF16_BAR)


def test_expert_ffn_grouped_uneven(fresh_moe):
    """Uneven offsets with empty experts: rows of experts 1 and 6."""
    import flashmoe_amd._ext as _ext

    cfg, g, ew, sc = _ffn_setup(fresh_moe, 103)
    rows = torch.randn(48, cfg["hidden_size"], generator=g).to(
        torch.bfloat16).cuda()
    offsets = np.array([0, 0, 16, 16, 16, 16, 16, 48, 48], dtype=np.int64)
    out = torch.zeros_like(rows)
    st = torch.cuda.current_stream().cuda_stream
    _ext.check(_ext.load().fm_expert_ffn_grouped(
        ctypes.c_void_p(st), ctypes.c_void_p(rows.data_ptr()),
        ctypes.c_void_p(offsets.ctypes.data), 8,
        ctypes.c_void_p(ew.data_ptr()), None, None,
        ctypes.c_void_p(out.data_ptr())), "fm_expert_ffn_grouped")
    torch.cuda.synchronize()
    assert_values(out[:16], _ffn_want(cfg, rows[:16], ew, sc, 1), "bf16",
                  "grouped[e1]", **BF16_BAR)
    assert_values(out[16:], _ffn_want(cfg, rows[16:], ew, sc, 6), "bf16",
                  "grouped[e6]", **BF16_BAR)


# --- dtype 5 (MX)

def test_mx_relu_small(fresh_moe):
    """128x128 tile, separate k_quant_mx pass."""
    run_scaled(fresh_moe, bar=MX_SMALL_BAR, torch_dtype=5)


def test_mx_gelu_with_biases(fresh_moe):
    """The shape of test_mx_fp8_gelu_bias."""
    cfg, path = make_cfg(torch_dtype=5, hidden_act=1, sequence_len=256,
                         hidden_size=128, intermediate_size=384,
                         capacity_factor=2)
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    sc = draw_scales(cfg)
    b_up, b_dn = draw_biases(cfg, seed=9)
    fresh_moe.set_weight_scales(sc)
    out = forward_raw(fresh_moe, cfg, x, gw, ew, b_up, b_dn)
    check(cfg, out, reference(cfg, x, gw, ew, sc, b_up, b_dn),
          bar=MX_SMALL_BAR)


def test_mx_in_epilogue_quantisation(fresh_moe):
    """The shape of test_mx_fp8_mid_geometry_epilogue_quant: the 128x256 tile
    quantises the scaled activations in its epilogue."""
    cfg, path = make_cfg(torch_dtype=5, sequence_len=2048, num_experts=256,
                         expert_top_k=2, hidden_size=128,
                         intermediate_size=256, capacity_factor=4)
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    sc = draw_scales(cfg)
    # the host's rule for the quantising 256-wide tile (mxWideN over pEC, P,
    # E): the up GEMM's 128x256 jobs fill the CUs. Restated so that this shape
    # cannot quietly become a copy of the small-shape case.
    S = cfg["sequence_len"] * cfg["mini_batch"]
    EC = -(-S // cfg["num_experts"]) * cfg["capacity_factor"] * 2
    jobs = -(-EC // 128) * (cfg["intermediate_size"] // 256) * cfg["num_experts"]
    assert cfg["intermediate_size"] >= 256 and jobs >= \
        torch.cuda.get_device_properties(0).multi_processor_count
    out = fresh_moe.moe_forward(x, gw, ew, weight_scales=sc)
    torch.cuda.synchronize()
    assert fresh_moe.get_weight_scales() is sc
    _assert_mx_values(out.view(S, -1), reference(cfg, x, gw, ew, sc)["moe_out"])


# --- behaviour

@pytest.mark.parametrize("dtype_code,act", [(4, 0), (4, 2), (5, 0)])
def test_ones_and_detach_are_bit_identical_to_no_scales(fresh_moe, dtype_code,
                                                        act):
    cfg, path = make_cfg(torch_dtype=dtype_code, hidden_act=act)
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    before = fresh_moe.moe_forward(x, gw, ew).clone()
    ones = torch.ones(n_records(cfg), record_len(cfg), device="cuda")
    fresh_moe.set_weight_scales(ones)
    with_ones = fresh_moe.moe_forward(x, gw, ew).clone()
    fresh_moe.set_weight_scales(draw_scales(cfg))
    scaled = fresh_moe.moe_forward(x, gw, ew).clone()
    fresh_moe.set_weight_scales(None)
    assert fresh_moe.get_weight_scales() is None
    after = fresh_moe.moe_forward(x, gw, ew).clone()
    torch.cuda.synchronize()
    assert torch.equal(with_ones, before)
    assert torch.equal(after, before)
    assert not torch.equal(scaled, before)


def test_graph_replay_sees_new_values_and_new_tensor(fresh_moe):
    """The forward graph is keyed on the scale pointer and the set-call
    generation. Every forward here has the same pointers (one fixed `out`,
    raw ABI) on a side stream - the default stream's handle is 0 and is never
    captured: the first is eager, the second captures and launches the graph,
    the rest replay it. Five identical forwards are bit-identical; values
    rewritten in place (same key: the replay reads the new contents) and a
    different tensor (new key: a replay of the old graph would read the old
    tensor) each give their own reference."""
    cfg, path = make_cfg(torch_dtype=4, hidden_act=2)
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    sc = draw_scales(cfg)
    fresh_moe.set_weight_scales(sc)
    S = cfg["sequence_len"] * cfg["mini_batch"]
    out = torch.empty(S, cfg["hidden_size"], dtype=torch.bfloat16,
                      device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())

    def forward():
        out.zero_()
        torch.cuda.synchronize()
        forward_raw(fresh_moe, cfg, x, gw, ew, out=out, stream=stream)
        return out.clone()

    outs = [forward() for _ in range(5)]
    check(cfg, outs[0], reference(cfg, x, gw, ew, sc))
    for i in range(1, 5):
        assert torch.equal(outs[i], outs[0]), f"forward {i} diverged"

    sc.copy_(draw_scales(cfg, seed=49))  # in place: same pointer, same graph
    torch.cuda.synchronize()
    got = forward()
    check(cfg, got, reference(cfg, x, gw, ew, sc, tag="seed49"), "in place")
    assert not torch.equal(got, outs[0])

    other = draw_scales(cfg, seed=50)
    assert other.data_ptr() != sc.data_ptr()
    fresh_moe.set_weight_scales(other)
    for i in range(3):  # eager, capture, replay under the new key
        got = forward()
        check(cfg, got, reference(cfg, x, gw, ew, other, tag="seed50"),
              f"other tensor[{i}]")

    fresh_moe.set_weight_scales(sc)  # the first pointer again, a new generation
    got = forward()
    check(cfg, got, reference(cfg, x, gw, ew, sc, tag="seed49"), "re-attached")

    fresh_moe.set_weight_scales(None)  # detached: no stale scaled graph
    no_scales = forward()
    ones = torch.ones_like(sc)
    check(cfg, no_scales, reference(cfg, x, gw, ew, ones, tag="ones"),
          "detached")


def test_refusals_through_the_abi(fresh_moe):
    import flashmoe_amd._ext as _ext

    lib = _ext.load()
    cfg, path = make_cfg(torch_dtype=2)
    fresh_moe.initialize(path, rank=0, world_size=1)
    sc = torch.ones(n_records(cfg), record_len(cfg), device="cuda")
    p = ctypes.c_void_p(sc.data_ptr())
    assert lib.fm_set_weight_scales(p, 1) == FM_ERR_UNSUPPORTED
    assert b"torch_dtype" in lib.fm_last_error()
    assert lib.fm_set_weight_scales(p, 2) == FM_ERR_UNSUPPORTED
    assert lib.fm_set_weight_scales(None, 0) == 0
    with pytest.raises(ValueError, match="torch_dtype"):
        fresh_moe.set_weight_scales(sc)
    fresh_moe.finalize()

    cfg, path = make_cfg(torch_dtype=4)
    fresh_moe.initialize(path, rank=0, world_size=1)
    assert lib.fm_set_weight_scales(p, 2) == FM_ERR_UNSUPPORTED
    assert b"128x128" in lib.fm_last_error()
    assert fresh_moe.get_weight_scales() is None  # refused calls attach nothing


def test_python_validation(fresh_moe):
    cfg, path = make_cfg(torch_dtype=4, hidden_act=2)
    fresh_moe.initialize(path, rank=0, world_size=1)
    n, SC = n_records(cfg), record_len(cfg)
    with pytest.raises(ValueError, match=rf"\[{n}, {SC}\]"):
        fresh_moe.set_weight_scales(torch.ones(n, SC - 256, device="cuda"))
    with pytest.raises(ValueError, match=rf"\[{n}, {SC}\]"):
        fresh_moe.set_weight_scales(
            torch.ones(n, SC, device="cuda", dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="CUDA"):
        fresh_moe.set_weight_scales(torch.ones(n, SC))
    with pytest.raises(ValueError, match=rf"\[{n}, {SC}\]"):
        fresh_moe.set_weight_scales(torch.ones(SC, n, device="cuda").t())
    assert fresh_moe.get_weight_scales() is None
    # after initialize, broadcast-only arguments take P and H from the config
    per_tensor = torch.full((n, 1), 2.0, device="cuda")
    packed = fresh_moe.pack_weight_scales(per_tensor, torch.tensor(0.5),
                                          per_tensor[:, 0])
    assert tuple(packed.shape) == (n, SC) and packed.is_cuda
    P = cfg["intermediate_size"]
    assert packed[:, :P].eq(2.0).all() and packed[:, P:P + 128].eq(0.5).all()
    fresh_moe.set_weight_scales(packed)
    assert fresh_moe.get_weight_scales() is packed


def test_get_reports_scales_attached_through_the_raw_abi(fresh_moe):
    import flashmoe_amd._ext as _ext

    cfg, path = make_cfg(torch_dtype=4)
    fresh_moe.initialize(path, rank=0, world_size=1)
    sc = draw_scales(cfg)
    _ext.check(_ext.load().fm_set_weight_scales(
        ctypes.c_void_p(sc.data_ptr()), 1), "fm_set_weight_scales")
    with pytest.raises(RuntimeError, match="fm_set_weight_scales"):
        fresh_moe.get_weight_scales()
    fresh_moe.set_weight_scales(sc)
    assert fresh_moe.get_weight_scales() is sc


# --- child-process cases: forced big-tile modes, persistent walk, FM_FUSED

# Runs in the child. argv[1]: JSON {cfgs: [cfg overrides], runs, fused}.
CHILD = r"""
import json, sys
import torch
from tests.test_gpu_parity import make_cfg
from tests.test_gpu_wscale import check, draw, draw_scales, reference
from flashmoe_amd import moe
import flashmoe_amd._ext as _ext

spec = json.loads(sys.argv[1])
for kw in spec["cfgs"]:
    cfg, path = make_cfg(**kw)
    moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    sc = draw_scales(cfg)
    if spec["fused"]:
        moe.moe_forward(x, gw, ew)
        torch.cuda.synchronize()
        assert _ext.load().fm_last_forward_fused() == 1, "FM_FUSED=1 not taken"
    moe.set_weight_scales(sc)
    ref = reference(cfg, x, gw, ew, sc)
    for run in range(spec["runs"]):
        out = moe.moe_forward(x, gw, ew)
        torch.cuda.synchronize()
        if spec["fused"]:
            assert _ext.load().fm_last_forward_fused() == 0, "fused path ran"
        check(cfg, out, ref, f"moe_out[act {cfg['hidden_act']}, run {run}]")
    moe.finalize()
print("CHILD OK")
"""


def run_child(env_extra, cfgs, runs=1, fused=False):
    env = dict(os.environ, PYTHONPATH=REPO_ROOT)
    for k in ("FM_FORCE_MODE", "FM_PERSIST_BLOCKS", "FM_PERSIST", "FM_FUSED",
              "FM_DECODE_FFN"):
        env.pop(k, None)
    env.update(env_extra)
    spec = {"cfgs": cfgs, "runs": runs, "fused": fused}
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(spec)],
                       capture_output=True, text=True, timeout=300,
                       cwd=REPO_ROOT, env=env)
    sys.stdout.write(r.stdout[-1500:])
    sys.stderr.write(r.stderr[-3000:])
    assert r.returncode == 0, f"child failed (rc {r.returncode})"
    assert "CHILD OK" in r.stdout


# test_gpu_gated's forced-mode shape: S=512, E=2, top-2, CF=2 (pEC = 1024 rows
# per expert, about half routed: partly filled and empty M tiles in every tile
# mode), H=192 / P=320 ragged against the 128- and 256-wide tiles. relu and
# SwiGLU run in the same child (the mode is cached per process, the config
# is not).
RAGGED = dict(torch_dtype=4, sequence_len=512, num_experts=2, expert_top_k=2,
              hidden_size=192, intermediate_size=320, capacity_factor=2)
RAGGED_BOTH = [dict(RAGGED, hidden_act=0), dict(RAGGED, hidden_act=2)]


@pytest.mark.parametrize("mode", [0, 1, 3, 4])
def test_forced_tile_modes(mode):
    run_child({"FM_FORCE_MODE": str(mode), "FM_FUSED": "0"}, RAGGED_BOTH)


def test_persistent_walk_three_blocks():
    """Three blocks walk all jobs of both experts: a scale vector loaded once
    per block instead of once per job would be another job's."""
    run_child({"FM_FORCE_MODE": "0", "FM_PERSIST_BLOCKS": "3",
               "FM_FUSED": "0"}, RAGGED_BOTH, runs=2)


def test_fused_request_runs_classic_path_with_scales():
    """FM_FUSED=1, dtype 4: fused without scales, the multi-kernel path (and
    the right values) with them."""
    run_child({"FM_FUSED": "1"},
              [dict(torch_dtype=4, hidden_act=1, sequence_len=256,
                    capacity_factor=2)], fused=True)
