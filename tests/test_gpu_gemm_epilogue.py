"""Big-tile expert GEMM prologue/epilogue: wide stores, hoisted row
addresses, per-wave routed count, double-buffered row metadata.

Every case runs its forward in a fresh child process, because the tile
mode (FM_FORCE_MODE) and the persistent-grid cap (FM_PERSIST_BLOCKS) are
cached at first use. The child compares against oracle.moe_oracle with
the project's bf16 bar (test_gpu_parity.assert_values: rtol 2e-2,
atol 2e-3 * scale), for the output and for the gate output.

All cases use capacity_factor 2: no expert overflows, so the kept set is
deterministic (DESIGN "flaky-test lesson").
"""
import json
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

from tests.conftest import REPO_ROOT

pytestmark = pytest.mark.gpu

# Runs in the child. argv[1]: JSON {cfg overrides, runs, bias, want_fused}.
CHILD = r"""
import ctypes, json, sys
import numpy as np
import torch
from oracle.moe_oracle import OracleConfig, moe_forward as oracle_forward
from tests.test_gpu_parity import assert_values, make_cfg
from flashmoe_amd import moe
import flashmoe_amd._ext as _ext
from flashmoe_amd.config import torch_dtype_of, weight_dtype_of

spec = json.loads(sys.argv[1])
cfg, path = make_cfg(**spec["cfg"])
moe.initialize(path, rank=0, world_size=1)
S = cfg["sequence_len"] * cfg["mini_batch"]
H, P, E = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_experts"]
dt, wdt = torch_dtype_of(cfg["torch_dtype"]), weight_dtype_of(cfg["torch_dtype"])
g = torch.Generator(device="cpu").manual_seed(47)
x = torch.randn(1, S, H, generator=g).to(dt).cuda()
gw = torch.randn(H, E, generator=g).to(dt).cuda()
ew = torch.randn(E, 2, P, H, generator=g).to(wdt).cuda()
b_up = b_dn = None
if spec["bias"]:
    b_up = torch.randn(E, P, generator=g).to(dt).cuda()
    b_dn = torch.randn(E, H, generator=g).to(dt).cuda()

element = {2: "bf16", 3: "fp16", 4: "bf16"}[cfg["torch_dtype"]]
ocfg = OracleConfig(num_experts=E, expert_top_k=cfg["expert_top_k"],
                    capacity_factor=cfg["capacity_factor"],
                    drop_tokens=cfg["drop_tokens"],
                    hidden_act=cfg["hidden_act"], element=element)
kw = {}
if spec["bias"]:
    kw = dict(b_up=b_up.float().cpu().numpy(), b_dn=b_dn.float().cpu().numpy())
ref = oracle_forward(x.view(S, H).float().cpu().numpy(),
                     gw.float().cpu().numpy().reshape(-1),
                     ew.float().cpu().numpy(), ocfg, **kw)
assert int(ref["eC"].sum()) == S * cfg["expert_top_k"]  # nothing dropped

lib = _ext.load()
st = torch.cuda.current_stream().cuda_stream
for run in range(spec["runs"]):
    if spec["bias"]:
        out = torch.empty(S, H, dtype=dt, device="cuda")
        gate_out = moe.gate_output()
        _ext.check(lib.fm_moe_forward(
            ctypes.c_void_p(st), ctypes.c_void_p(x.data_ptr()),
            ctypes.c_void_p(gw.data_ptr()), ctypes.c_void_p(ew.data_ptr()),
            ctypes.c_void_p(b_up.data_ptr()), ctypes.c_void_p(b_dn.data_ptr()),
            ctypes.c_void_p(gate_out.data_ptr()),
            ctypes.c_void_p(out.data_ptr()), S), "fm_moe_forward")
    else:
        out = moe.moe_forward(x, gw, ew)
        gate_out = moe.gate_output()
    torch.cuda.synchronize()
    # the bf16 bar for values and gate outputs, fp16 included
    assert_values(gate_out, ref["gate_out"], element, f"gate_out[run {run}]",
                  rtol=2e-2, atol_scale=2e-3)
    assert_values(out.view(S, H), ref["moe_out"], element,
                  f"moe_out[run {run}]", rtol=2e-2, atol_scale=2e-3)
moe.finalize()
print("CHILD OK")
"""


def run_child(env_extra, runs=1, bias=False, **cfg):
    cfg.setdefault("capacity_factor", 2)
    env = dict(os.environ, PYTHONPATH=REPO_ROOT)
    for k in ("FM_FORCE_MODE", "FM_PERSIST_BLOCKS", "FM_PERSIST", "FM_FUSED"):
        env.pop(k, None)
    env.update(env_extra)
    spec = {"cfg": cfg, "runs": runs, "bias": bias}
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(spec)],
                       capture_output=True, text=True, timeout=300,
                       cwd=REPO_ROOT, env=env)
    sys.stdout.write(r.stdout[-1500:])
    sys.stderr.write(r.stderr[-3000:])
    assert r.returncode == 0, f"child failed (rc {r.returncode})"
    assert "CHILD OK" in r.stdout


# S=512, E=2, top-2, CF=2: pEC = 1024 rows per expert of which ~512 are
# routed, so every forced tile mode sees a partly filled M tile and wholly
# empty M tiles; H=192 / P=320 are ragged against 128 and 256, so the last
# N tile has column groups that lie past N (and the B-row clamp) in both
# the up (PHASE 0) and the down (PHASE 1) GEMM.
RAGGED = dict(sequence_len=512, num_experts=2, expert_top_k=2,
              hidden_size=192, intermediate_size=320)


@pytest.mark.parametrize("mode", [0, 1, 3, 4])
def test_forced_tile_modes_bf16(mode):
    run_child({"FM_FORCE_MODE": str(mode), "FM_FUSED": "0"}, **RAGGED)


def test_forced_tile_mode0_fp16():
    run_child({"FM_FORCE_MODE": "0", "FM_FUSED": "0"}, torch_dtype=3, **RAGGED)


@pytest.mark.parametrize("mode", [0, 4])
def test_persistent_walk_three_blocks(mode):
    """FM_PERSIST_BLOCKS=3: each block walks several jobs, empty and
    non-empty ones following each other in both orders (the metadata
    copy flips only after a job that ran). Three forwards in one process,
    each compared: nothing may be carried from one forward to the next."""
    run_child({"FM_FORCE_MODE": str(mode), "FM_PERSIST_BLOCKS": "3",
               "FM_FUSED": "0"}, runs=3, **RAGGED)


SMALL = dict(sequence_len=256, num_experts=2, hidden_size=128,
             intermediate_size=256)


def test_top1_direct_store():
    """top-1: unscaled, the down epilogue writes moe_out rows directly."""
    run_child({"FM_FORCE_MODE": "0", "FM_FUSED": "0"}, expert_top_k=1, **SMALL)


def test_bias_gelu():
    run_child({"FM_FORCE_MODE": "0", "FM_FUSED": "0"}, bias=True,
              expert_top_k=2, hidden_act=1, **SMALL)


def test_fp8_weights():
    run_child({"FM_FORCE_MODE": "0", "FM_FUSED": "0"}, expert_top_k=2,
              torch_dtype=4, **SMALL)


def test_fused_kernel_sc1_wide_stores():
    """The single-launch kernel: its up/down epilogues publish through
    agent-scope write-through stores, now 8 bytes wide."""
    run_child({"FM_FUSED": "1"}, sequence_len=1024, num_experts=8,
              expert_top_k=2, hidden_size=256, intermediate_size=512)
