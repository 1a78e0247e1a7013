"""Shared experts (num_shared_experts) on the GPU against
tests/shared_ref.py.

Bars are the project's own (test_gpu_parity.assert_values: bf16/fp16
rtol 2e-2, atol 2e-3 * scale; fp32 1e-5), every element inside. Inputs are
drawn x, gw, weights from Generator().manual_seed(47) as
test_gpu_gated.draw does, with E + nSh weight slabs: x and gw come first,
so the routing does not depend on nSh.

Base shape S=128, H=128, P=256, E=8, top-2, CF=1, drop: EC = 32, so each
shared expert is FOUR 32-row z-slices. S=128 is one routing tile, so the
kept set under drops is deterministic. With seed 47, top-1 drops 11 tokens
(all of them wholly dropped), top-2 drops 13 slots and leaves 2 tokens
wholly dropped (pinned on the CPU in tests/test_shared_cpu.py).

The forced tile modes, the persistent-grid cap and FM_FUSED are cached at
first use, so those cases each run in one fresh child process.
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
from tests.shared_ref import shared_moe_forward
from tests.test_gpu_parity import assert_values, fresh_moe, make_cfg  # noqa: F401

pytestmark = pytest.mark.gpu

ELEMENT = {0: "fp32", 1: "fp32", 2: "bf16", 3: "fp16", 4: "bf16"}
FM_ERR_UNSUPPORTED = -4


def bar(element):
    # assert_values applies its fp32 bar to everything that is not "bf16";
    # fp16 carries the bf16 bar (as in test_gpu_gated)
    return {} if element == "fp32" else dict(rtol=2e-2, atol_scale=2e-3)


def draw(cfg, seed=47):
    """test_gpu_gated.draw with E + nSh expert slabs (shared ones last)."""
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


def reference(cfg, x, gw, ew, b_dn=None):
    S = cfg["sequence_len"] * cfg["mini_batch"]
    ocfg = OracleConfig(
        num_experts=cfg["num_experts"], expert_top_k=cfg["expert_top_k"],
        capacity_factor=cfg["capacity_factor"], drop_tokens=cfg["drop_tokens"],
        hidden_act=cfg["hidden_act"], element=ELEMENT[cfg["torch_dtype"]])
    return shared_moe_forward(
        x.view(S, -1).float().cpu().numpy(),
        gw.float().cpu().numpy().reshape(-1), ew.float().cpu().numpy(), ocfg,
        cfg.get("num_shared_experts", 0),
        b_dn.float().cpu().numpy() if b_dn is not None else None)


def check(cfg, out, gate_out, ref, what="moe_out"):
    S = cfg["sequence_len"] * cfg["mini_batch"]
    element = ELEMENT[cfg["torch_dtype"]]
    if gate_out is not None:
        assert_values(gate_out, ref["gate_out"], element, "gate_out",
                      **bar(element))
    assert_values(out.view(S, -1), ref["moe_out"], element, what,
                  **bar(element))


def run_shared(moe, **kw):
    kw.setdefault("num_shared_experts", 1)
    cfg, path = make_cfg(**kw)
    moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    out = moe.moe_forward(x, gw, ew)
    gate_out = moe.gate_output().clone()
    torch.cuda.synchronize()
    import flashmoe_amd._ext as _ext

    assert _ext.load().fm_last_forward_fused() == 0
    assert moe.get_num_local_experts() == cfg["num_experts"]
    assert moe.get_num_shared_experts() == cfg["num_shared_experts"]
    ref = reference(cfg, x, gw, ew)
    check(cfg, out, gate_out, ref)
    return cfg, out, ref


# --- in-process: the base shape (128x128 synchronous tile / fp32 kernel)

@pytest.mark.parametrize("dtype_code", [2, 3, 0, 4])
def test_swiglu_one_shared(fresh_moe, dtype_code):
    _, _, ref = run_shared(fresh_moe, hidden_act=2, torch_dtype=dtype_code)
    assert float(np.abs(ref["shared_out"]).max()) > 1.0  # not vacuous


def test_relu_one_shared(fresh_moe):
    """Ungated experts: [E + 1, 2, P, H]."""
    run_shared(fresh_moe, hidden_act=0)


def test_geglu_two_shared(fresh_moe):
    """Slots k and k + 1, weight experts E and E + 1."""
    run_shared(fresh_moe, hidden_act=3, num_shared_experts=2)


def test_top3_ragged_last_slice(fresh_moe):
    """top-3: EC = 48, so the 128 tokens are slices of 48, 48 and 32 rows."""
    run_shared(fresh_moe, hidden_act=2, expert_top_k=3)


def test_top1_dropped_tokens_keep_shared_term(fresh_moe):
    """top-1: the direct-store path switches to combine slots, the K = 1
    combine runs, and the tokens whose only routed slot was dropped still
    receive their shared term (no zeroed moe_out to lean on)."""
    cfg, out, ref = run_shared(fresh_moe, hidden_act=2, expert_top_k=1)
    gone = ~ref["kept"].any(axis=1)
    assert int(gone.sum()) == 11  # the reference really has dropped tokens
    assert np.array_equal(ref["moe_out"][gone], ref["shared_out"][gone])
    got = out.view(128, -1).float().cpu().numpy()
    assert np.abs(got[gone]).max() > 1.0


def test_top2_has_dropped_tokens(fresh_moe):
    cfg, out, ref = run_shared(fresh_moe, hidden_act=2)
    assert int((~ref["kept"]).sum()) == 13
    assert int((~ref["kept"].any(axis=1)).sum()) == 2


def test_no_drop_one_slice_spanning_m_tiles(fresh_moe):
    """drop_tokens 0, S = 256: EC = 512 >= S, so the shared expert is ONE
    slice of 256 rows - two 128-row M tiles of the same z."""
    cfg, _, ref = run_shared(fresh_moe, hidden_act=2, drop_tokens=0,
                             sequence_len=256)
    assert int(ref["eC"].sum()) == 256 * 2  # nothing dropped


def test_down_bias_through_the_raw_abi(fresh_moe):
    """b_dn is indexed by weight-expert id: [E + nSh, H]."""
    import flashmoe_amd._ext as _ext

    cfg, path = make_cfg(hidden_act=2, num_shared_experts=1)
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    S, H, E = 128, cfg["hidden_size"], cfg["num_experts"]
    g = torch.Generator().manual_seed(321)
    b_dn = torch.randn(E + 1, H, generator=g).to(torch.bfloat16).cuda()
    out = torch.empty(S, H, dtype=torch.bfloat16, device="cuda")
    gate_out = fresh_moe.gate_output()
    lib = _ext.load()
    st = torch.cuda.current_stream().cuda_stream
    _ext.check(lib.fm_moe_forward(
        ctypes.c_void_p(st), ctypes.c_void_p(x.data_ptr()),
        ctypes.c_void_p(gw.data_ptr()), ctypes.c_void_p(ew.data_ptr()),
        None, ctypes.c_void_p(b_dn.data_ptr()),
        ctypes.c_void_p(gate_out.data_ptr()), ctypes.c_void_p(out.data_ptr()),
        S), "fm_moe_forward")
    torch.cuda.synchronize()
    ref = reference(cfg, x, gw, ew, b_dn)
    check(cfg, out, None, ref, "moe_out(b_dn)")
    # the shared expert's own bias row matters
    no_bias = reference(cfg, x, gw, ew)
    assert np.abs(ref["shared_out"] - no_bias["shared_out"]).max() > 0.5


# --- the two halves in isolation

@pytest.mark.parametrize("k", [2, 1])
def test_routed_part_untouched(fresh_moe, k):
    """Shared slabs all zero: moe_out is torch.equal to a forward of the
    nSh = 0 config on the same routed weights (bf16, E = 8, inference: the
    deterministic gate, one routing tile)."""
    cfg1, path1 = make_cfg(hidden_act=2, expert_top_k=k, num_shared_experts=1)
    x, gw, ew = draw(cfg1)
    E = cfg1["num_experts"]
    ew[E:] = 0
    fresh_moe.initialize(path1, rank=0, world_size=1)
    with_shared = fresh_moe.moe_forward(x, gw, ew).clone()
    torch.cuda.synchronize()
    fresh_moe.finalize()
    cfg0, path0 = make_cfg(hidden_act=2, expert_top_k=k)
    fresh_moe.initialize(path0, rank=0, world_size=1)
    plain = fresh_moe.moe_forward(x, gw, ew[:E].contiguous()).clone()
    torch.cuda.synchronize()
    assert plain.float().abs().max() > 1.0
    assert torch.equal(with_shared, plain)


def test_shared_part_alone(fresh_moe):
    """Routed slabs all zero: every row - the wholly dropped tokens
    included - is the reference's shared sum."""
    cfg, path = make_cfg(hidden_act=2, num_shared_experts=2)
    x, gw, ew = draw(cfg)
    E = cfg["num_experts"]
    ew[:E] = 0
    fresh_moe.initialize(path, rank=0, world_size=1)
    out = fresh_moe.moe_forward(x, gw, ew)
    torch.cuda.synchronize()
    ref = reference(cfg, x, gw, ew)
    assert int((~ref["kept"].any(axis=1)).sum()) == 2
    from oracle.moe_oracle import bf16_round

    assert np.array_equal(ref["moe_out"], bf16_round(ref["shared_out"]))
    assert np.abs(ref["shared_out"]).min(axis=1).max() > 0
    check(cfg, out, None, ref, "moe_out(shared only)")


# --- the static routing tail survives every forward

def five_identical_calls(moe, cfg, x, gw, ew):
    """Five fm_moe_forward calls with identical pointers on a side stream:
    the first is eager, the second captures the graph and launches it, the
    rest replay it."""
    import flashmoe_amd._ext as _ext

    lib = _ext.load()
    S = cfg["sequence_len"] * cfg["mini_batch"]
    out = torch.empty_like(x)
    gate_out = moe.gate_output()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(5):
        out.zero_()
        torch.cuda.synchronize()
        _ext.check(lib.fm_moe_forward(
            ctypes.c_void_p(stream.cuda_stream), ctypes.c_void_p(x.data_ptr()),
            ctypes.c_void_p(gw.data_ptr()), ctypes.c_void_p(ew.data_ptr()),
            None, None, ctypes.c_void_p(gate_out.data_ptr()),
            ctypes.c_void_p(out.data_ptr()), S), "fm_moe_forward")
        torch.cuda.synchronize()
        outs.append(out.clone())
    return outs


def test_static_tail_eager_capture_replay(fresh_moe):
    cfg, path = make_cfg(hidden_act=2, num_shared_experts=1)
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    ref = reference(cfg, x, gw, ew)
    outs = five_identical_calls(fresh_moe, cfg, x, gw, ew)
    for i, o in enumerate(outs):
        check(cfg, o, None, ref, f"moe_out[call {i}]")
        assert torch.equal(o, outs[0]), f"call {i} differs from call 0"


# --- child-process cases

# Runs in the child. argv[1]: JSON {cfg overrides, runs, want_classic, five}.
CHILD = r"""
import json, sys
import torch
from tests.test_gpu_parity import make_cfg
from tests.test_gpu_shared import check, draw, five_identical_calls, reference
from flashmoe_amd import moe
import flashmoe_amd._ext as _ext

spec = json.loads(sys.argv[1])
cfg, path = make_cfg(**spec["cfg"])
moe.initialize(path, rank=0, world_size=1)
x, gw, ew = draw(cfg)
ref = reference(cfg, x, gw, ew)
if spec["five"]:
    for i, o in enumerate(five_identical_calls(moe, cfg, x, gw, ew)):
        check(cfg, o, None, ref, f"moe_out[call {i}]")
for run in range(spec["runs"]):
    out = moe.moe_forward(x, gw, ew)
    gate_out = moe.gate_output()
    torch.cuda.synchronize()
    if spec["want_classic"]:
        assert _ext.load().fm_last_forward_fused() == 0, "fused path ran"
    check(cfg, out, gate_out, ref, f"moe_out[run {run}]")
moe.finalize()
print("CHILD OK")
"""


def run_child(env_extra, runs=1, want_classic=False, five=False, **cfg):
    cfg.setdefault("hidden_act", 2)
    cfg.setdefault("num_shared_experts", 1)
    env = dict(os.environ, PYTHONPATH=REPO_ROOT)
    for k in ("FM_FORCE_MODE", "FM_PERSIST_BLOCKS", "FM_PERSIST", "FM_FUSED",
              "FM_GATE_FUSED"):
        env.pop(k, None)
    env.update(env_extra)
    spec = {"cfg": cfg, "runs": runs, "want_classic": want_classic,
            "five": five}
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(spec)],
                       capture_output=True, text=True, timeout=300,
                       cwd=REPO_ROOT, env=env)
    sys.stdout.write(r.stdout[-1500:])
    sys.stderr.write(r.stderr[-3000:])
    assert r.returncode == 0, f"child failed (rc {r.returncode})"
    assert "CHILD OK" in r.stdout


def test_static_tail_two_kernel_gate():
    """FM_GATE_FUSED=0: the logits kernel zeroes E counts and the route
    kernel refills them; the tail must survive that gate too. Its routing
    uses atomics, so the five calls are compared to the reference only."""
    run_child({"FM_GATE_FUSED": "0"}, runs=0, five=True)


# H=192 / P=320 are ragged against every tile; S=256, E=8, top-2, CF=2:
# EC = pEC = 128 and nothing is dropped, so the shared expert is two full
# 128-row slices beside eight partly filled routed ones.
RAGGED = dict(sequence_len=256, num_experts=8, expert_top_k=2,
              capacity_factor=2, hidden_size=192, intermediate_size=320)


@pytest.mark.parametrize("mode", [0, 1, 3, 4])
def test_forced_tile_modes(mode):
    run_child({"FM_FORCE_MODE": str(mode), "FM_FUSED": "0"}, **RAGGED)


def test_persistent_walk_three_blocks():
    """Three blocks walk every job of both launches, routed and shared
    slices alike; three forwards, each compared."""
    run_child({"FM_FORCE_MODE": "4", "FM_PERSIST_BLOCKS": "3",
               "FM_FUSED": "0"}, runs=3, **RAGGED)


def test_persistent_walk_over_routed_empty_and_shared_jobs():
    """The same walk without drops (EC = pEC = 512 = four 128-row M tiles
    per z): a routed expert fills about half of its first tile and leaves
    three empty, the shared slice fills two and leaves two empty, so one
    block meets routed, empty and shared jobs in turn."""
    run_child({"FM_FORCE_MODE": "4", "FM_PERSIST_BLOCKS": "3",
               "FM_FUSED": "0"}, runs=2,
              **dict(RAGGED, drop_tokens=0, capacity_factor=1))


def test_fused_request_runs_classic_path_with_shared_experts():
    """FM_FUSED=1 on a plain (relu) config that would otherwise take the
    single-launch kernel: with shared experts the forward must match and
    must have taken the multi-kernel path."""
    run_child({"FM_FUSED": "1"}, want_classic=True, hidden_act=0, **RAGGED)


def test_fused_request_runs_classic_path_swiglu():
    run_child({"FM_FUSED": "1"}, want_classic=True, **RAGGED)


# --- refusals

def _fm_config(**kw):
    import flashmoe_amd._ext as _ext

    base = dict(num_experts=8, expert_top_k=2, capacity_factor=1,
                drop_tokens=1, hidden_act=2, hidden_size=128,
                intermediate_size=256, sequence_len=128, mini_batch=1,
                dtype=2, is_training=0, num_shared_experts=1)
    base.update(kw)
    return _ext.FMConfig(**base)


@pytest.mark.parametrize("kw, world", [
    (dict(dtype=5, hidden_act=0), 1),
    (dict(dtype=5), 1),
    (dict(), 2),
    (dict(num_shared_experts=5), 1),
    (dict(num_shared_experts=-1), 1),
])
def test_initialize_refuses(kw, world):
    import flashmoe_amd._ext as _ext

    lib = _ext.load()
    c = _fm_config(**kw)
    assert lib.fm_initialize(ctypes.byref(c), 0, world) == FM_ERR_UNSUPPORTED
    assert b"num_shared_experts" in lib.fm_last_error()
    assert lib.fm_get_num_shared_experts() == -1  # nothing was initialized


def test_routed_only_tensor_is_refused(fresh_moe):
    cfg, path = make_cfg(hidden_act=2, num_shared_experts=1)
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    with pytest.raises(ValueError, match="num_shared_experts"):
        fresh_moe.moe_forward(x, gw, ew[:8].contiguous())
