"""Gated experts (hidden_act 2 SwiGLU / 3 GeGLU, [nLx, 3, P, H] weights)
on the GPU against tests/gated_ref.py.

Bars are the project's own (test_gpu_parity.assert_values: bf16/fp16
rtol 2e-2, atol 2e-3 * scale; fp32 1e-5), every element inside. Inputs
are drawn x, gw, weights from Generator().manual_seed(47) like
test_gpu_parity.run_pair. capacity_factor 2 wherever S > 128: nothing is
dropped, so the kept set is deterministic.

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
from tests.gated_ref import gated_expert_ffn, gated_moe_forward
from tests.test_gpu_parity import assert_values, fresh_moe, make_cfg  # noqa: F401

pytestmark = pytest.mark.gpu

ELEMENT = {0: "fp32", 1: "fp32", 2: "bf16", 3: "fp16", 4: "bf16"}
FM_ERR_UNSUPPORTED = -4


def bar(element):
    # assert_values applies its fp32 bar to everything that is not "bf16";
    # fp16 carries the bf16 bar (as in test_gpu_gemm_epilogue)
    return {} if element == "fp32" else dict(rtol=2e-2, atol_scale=2e-3)


def draw(cfg, seed=47):
    from flashmoe_amd.config import (expert_mats, torch_dtype_of,
                                     weight_dtype_of)

    H, P, E = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_experts"]
    dt = torch_dtype_of(cfg["torch_dtype"])
    wdt = weight_dtype_of(cfg["torch_dtype"])
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(cfg["mini_batch"], cfg["sequence_len"], H,
                    generator=g).to(dt).cuda()
    gw = torch.randn(H, E, generator=g).to(dt).cuda()
    ew = torch.randn(E, expert_mats(cfg["hidden_act"]), P, H,
                     generator=g).to(wdt).cuda()
    return x, gw, ew


def reference(cfg, x, gw, ew):
    S = cfg["sequence_len"] * cfg["mini_batch"]
    ocfg = OracleConfig(
        num_experts=cfg["num_experts"], expert_top_k=cfg["expert_top_k"],
        capacity_factor=cfg["capacity_factor"], drop_tokens=cfg["drop_tokens"],
        hidden_act=cfg["hidden_act"], element=ELEMENT[cfg["torch_dtype"]])
    ref = gated_moe_forward(
        x.view(S, -1).float().cpu().numpy(),
        gw.float().cpu().numpy().reshape(-1), ew.float().cpu().numpy(), ocfg)
    if S > 128:
        assert int(ref["eC"].sum()) == S * cfg["expert_top_k"]  # none dropped
    return ref


def run_gated(moe, **kw):
    cfg, path = make_cfg(**kw)
    moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    out = moe.moe_forward(x, gw, ew)
    gate_out = moe.gate_output().clone()
    torch.cuda.synchronize()
    ref = reference(cfg, x, gw, ew)
    S = cfg["sequence_len"] * cfg["mini_batch"]
    element = ELEMENT[cfg["torch_dtype"]]
    assert_values(gate_out, ref["gate_out"], element, "gate_out", **bar(element))
    assert_values(out.view(S, -1), ref["moe_out"], element, "moe_out",
                  **bar(element))


# --- in-process: small shapes (the 128x128 synchronous tile / fp32 kernel)

@pytest.mark.parametrize("dtype_code", [2, 3, 0, 4])
def test_swiglu_default_shape(fresh_moe, dtype_code):
    run_gated(fresh_moe, hidden_act=2, torch_dtype=dtype_code)


def test_geglu_bf16(fresh_moe):
    run_gated(fresh_moe, hidden_act=3)


def test_swiglu_top1_bf16(fresh_moe):
    run_gated(fresh_moe, hidden_act=2, expert_top_k=1)


def test_swiglu_ragged_bf16(fresh_moe):
    """H=192 / P=320: the effective N = 640 is ragged against the 128-wide
    tile, so the per-half B-row clamp and the P column guard both act."""
    run_gated(fresh_moe, hidden_act=2, hidden_size=192, intermediate_size=320,
              sequence_len=256, capacity_factor=2)


def _ffn_setup(moe, seed):
    cfg, path = make_cfg(hidden_act=2)
    moe.initialize(path, rank=0, world_size=1)
    H, P, E = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_experts"]
    g = torch.Generator().manual_seed(seed)
    ew = torch.randn(E, 3, P, H, generator=g).to(torch.bfloat16).cuda()
    return cfg, g, ew


def _ffn_want(rows, ew, e):
    w = ew[e].float().cpu().numpy()
    return gated_expert_ffn(rows.float().cpu().numpy(), w[0],
                            w[1].reshape(-1), w[2], 2, "bf16")


def test_expert_ffn_packed_rows(fresh_moe):
    """fm_expert_ffn for local expert 3: a 2*P*H expert stride would read
    another expert's slabs."""
    import flashmoe_amd._ext as _ext

    cfg, g, ew = _ffn_setup(fresh_moe, 99)
    rows = torch.randn(64, cfg["hidden_size"], generator=g).to(
        torch.bfloat16).cuda()
    out = torch.empty_like(rows)
    lib = _ext.load()
    st = torch.cuda.current_stream().cuda_stream
    _ext.check(lib.fm_expert_ffn(
        ctypes.c_void_p(st), ctypes.c_void_p(rows.data_ptr()),
        ctypes.c_void_p(ew.data_ptr()), None, None,
        ctypes.c_void_p(out.data_ptr()), 64, 3), "fm_expert_ffn")
    torch.cuda.synchronize()
    assert_values(out, _ffn_want(rows, ew, 3), "bf16", "expert_ffn(gated)")


def test_expert_ffn_segments(fresh_moe):
    """fm_expert_ffn_segments: two [EC, H] segments mapped to experts 5, 1."""
    import flashmoe_amd._ext as _ext

    cfg, g, ew = _ffn_setup(fresh_moe, 101)
    H, EC = cfg["hidden_size"], 32  # EC = ceil(128/8) * CF 1 * top-2
    rows = torch.randn(2, EC, H, generator=g).to(torch.bfloat16).cuda()
    seg = torch.tensor([5, 1], dtype=torch.int32, device="cuda")
    out = torch.empty_like(rows)
    lib = _ext.load()
    st = torch.cuda.current_stream().cuda_stream
    _ext.check(lib.fm_expert_ffn_segments(
        ctypes.c_void_p(st), ctypes.c_void_p(rows.data_ptr()),
        ctypes.c_void_p(seg.data_ptr()), 2, ctypes.c_void_p(ew.data_ptr()),
        ctypes.c_void_p(out.data_ptr())), "fm_expert_ffn_segments")
    torch.cuda.synchronize()
    for s, e in enumerate((5, 1)):
        assert_values(out[s], _ffn_want(rows[s], ew, e), "bf16",
                      f"ffn_segments(gated)[seg {s}]")


def test_expert_ffn_grouped(fresh_moe):
    """fm_expert_ffn_grouped walks fm_expert_ffn per local expert."""
    import flashmoe_amd._ext as _ext

    cfg, g, ew = _ffn_setup(fresh_moe, 103)
    rows = torch.randn(48, cfg["hidden_size"], generator=g).to(
        torch.bfloat16).cuda()
    offsets = np.array([0, 0, 16, 16, 16, 16, 16, 48, 48], dtype=np.int64)
    out = torch.zeros_like(rows)
    lib = _ext.load()
    st = torch.cuda.current_stream().cuda_stream
    _ext.check(lib.fm_expert_ffn_grouped(
        ctypes.c_void_p(st), ctypes.c_void_p(rows.data_ptr()),
        ctypes.c_void_p(offsets.ctypes.data), 8,
        ctypes.c_void_p(ew.data_ptr()), None, None,
        ctypes.c_void_p(out.data_ptr())), "fm_expert_ffn_grouped")
    torch.cuda.synchronize()
    assert_values(out[:16], _ffn_want(rows[:16], ew, 1), "bf16", "grouped[e1]")
    assert_values(out[16:], _ffn_want(rows[16:], ew, 6), "bf16", "grouped[e6]")


# --- error behaviour

def test_gated_rejects_up_bias(fresh_moe):
    import flashmoe_amd._ext as _ext

    cfg, path = make_cfg(hidden_act=2)
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    S, H, P, E = 128, 128, 256, 8
    b_up = torch.zeros(E, P, dtype=torch.bfloat16, device="cuda")
    out = torch.empty(S, H, dtype=torch.bfloat16, device="cuda")
    gate_out = fresh_moe.gate_output()
    lib = _ext.load()
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.fm_moe_forward(
        ctypes.c_void_p(st), ctypes.c_void_p(x.data_ptr()),
        ctypes.c_void_p(gw.data_ptr()), ctypes.c_void_p(ew.data_ptr()),
        ctypes.c_void_p(b_up.data_ptr()), None,
        ctypes.c_void_p(gate_out.data_ptr()), ctypes.c_void_p(out.data_ptr()),
        S)
    assert rc == FM_ERR_UNSUPPORTED
    assert b"b_up" in lib.fm_last_error()
    rows = torch.zeros(64, H, dtype=torch.bfloat16, device="cuda")
    rc = lib.fm_expert_ffn(
        ctypes.c_void_p(st), ctypes.c_void_p(rows.data_ptr()),
        ctypes.c_void_p(ew.data_ptr()), ctypes.c_void_p(b_up.data_ptr()), None,
        ctypes.c_void_p(out.data_ptr()), 64, 0)
    assert rc == FM_ERR_UNSUPPORTED
    torch.cuda.synchronize()


def test_gated_config_rejects_two_slab_weights(fresh_moe):
    cfg, path = make_cfg(hidden_act=2)
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    with pytest.raises(ValueError, match=r"\[nLx, 3, P, H\]"):
        fresh_moe.moe_forward(x, gw, ew[:, :2].contiguous())


def test_plain_config_rejects_three_slab_weights(fresh_moe):
    cfg, path = make_cfg(hidden_act=0)
    fresh_moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    ew3 = torch.cat([ew, ew[:, :1]], dim=1).contiguous()
    with pytest.raises(ValueError, match=r"\[nLx, 2, P, H\]"):
        fresh_moe.moe_forward(x, gw, ew3)


def test_gated_mx_rejected_at_initialize():
    """The C-ABI itself refuses gated + dtype 5 (config.py refuses it
    earlier on the Python path)."""
    import flashmoe_amd._ext as _ext

    lib = _ext.load()
    c = _ext.FMConfig(num_experts=8, expert_top_k=2, capacity_factor=1,
                      drop_tokens=1, hidden_act=2, hidden_size=128,
                      intermediate_size=256, sequence_len=128, mini_batch=1,
                      dtype=5, is_training=0)
    assert lib.fm_initialize(ctypes.byref(c), 0, 1) == FM_ERR_UNSUPPORTED
    assert b"hidden_act" in lib.fm_last_error()


# --- child-process cases: forced big-tile modes, persistent walk, FM_FUSED

# Runs in the child. argv[1]: JSON {cfg overrides, runs, want_classic}.
CHILD = r"""
import json, sys
import torch
from tests.test_gpu_parity import assert_values, make_cfg
from tests.test_gpu_gated import ELEMENT, bar, draw, reference
from flashmoe_amd import moe
import flashmoe_amd._ext as _ext

spec = json.loads(sys.argv[1])
cfg, path = make_cfg(**spec["cfg"])
moe.initialize(path, rank=0, world_size=1)
S = cfg["sequence_len"] * cfg["mini_batch"]
x, gw, ew = draw(cfg)
ref = reference(cfg, x, gw, ew)
element = ELEMENT[cfg["torch_dtype"]]
for run in range(spec["runs"]):
    out = moe.moe_forward(x, gw, ew)
    gate_out = moe.gate_output()
    torch.cuda.synchronize()
    if spec["want_classic"]:
        assert _ext.load().fm_last_forward_fused() == 0, "fused path ran"
    assert_values(gate_out, ref["gate_out"], element, f"gate_out[run {run}]",
                  **bar(element))
    assert_values(out.view(S, -1), ref["moe_out"], element,
                  f"moe_out[run {run}]", **bar(element))
moe.finalize()
print("CHILD OK")
"""


def run_child(env_extra, runs=1, want_classic=False, **cfg):
    cfg.setdefault("capacity_factor", 2)
    cfg.setdefault("hidden_act", 2)
    env = dict(os.environ, PYTHONPATH=REPO_ROOT)
    for k in ("FM_FORCE_MODE", "FM_PERSIST_BLOCKS", "FM_PERSIST", "FM_FUSED"):
        env.pop(k, None)
    env.update(env_extra)
    spec = {"cfg": cfg, "runs": runs, "want_classic": want_classic}
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(spec)],
                       capture_output=True, text=True, timeout=300,
                       cwd=REPO_ROOT, env=env)
    sys.stdout.write(r.stdout[-1500:])
    sys.stderr.write(r.stderr[-3000:])
    assert r.returncode == 0, f"child failed (rc {r.returncode})"
    assert "CHILD OK" in r.stdout


# S=512, E=2, top-2, CF=2: pEC = 1024 rows per expert, about half routed,
# so every tile mode sees partly filled and wholly empty M tiles. P=320:
# the effective N = 640 is two full 256-wide tiles plus a half tile (five
# 128-wide ones), so the last tile's gate AND up halves both run past
# P - the per-half clamp and the ragged epilogue.
RAGGED = dict(sequence_len=512, num_experts=2, expert_top_k=2,
              hidden_size=192, intermediate_size=320)


@pytest.mark.parametrize("mode", [0, 1, 3, 4])
def test_forced_tile_modes_swiglu_bf16(mode):
    run_child({"FM_FORCE_MODE": str(mode), "FM_FUSED": "0"}, **RAGGED)


def test_forced_mode0_swiglu_fp16():
    run_child({"FM_FORCE_MODE": "0", "FM_FUSED": "0"}, torch_dtype=3, **RAGGED)


def test_forced_mode0_swiglu_fp8_weights():
    run_child({"FM_FORCE_MODE": "0", "FM_FUSED": "0"}, torch_dtype=4, **RAGGED)


def test_forced_mode0_geglu_bf16():
    run_child({"FM_FORCE_MODE": "0", "FM_FUSED": "0"}, hidden_act=3, **RAGGED)


def test_persistent_walk_three_blocks_swiglu():
    """Three blocks walk all jobs; three forwards, each compared."""
    run_child({"FM_FORCE_MODE": "0", "FM_PERSIST_BLOCKS": "3",
               "FM_FUSED": "0"}, runs=3, **RAGGED)


def test_fused_request_runs_classic_path_when_gated():
    """FM_FUSED=1 with a gated config: the forward must match and must
    have taken the multi-kernel path (fm_last_forward_fused() == 0)."""
    run_child({"FM_FUSED": "1"}, want_classic=True, sequence_len=1024,
              num_experts=8, expert_top_k=2, hidden_size=256,
              intermediate_size=512)
