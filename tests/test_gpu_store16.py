"""16-byte epilogue stores of the big-tile expert GEMMs, and the
token-group form of k_cast_combine.

The epilogue exchanges the packed dwords of a fragment pair with
v_permlane16_swap so that a lane owns eight consecutive output columns.
The lane-to-column map after the swap was derived from the instruction's
definition; the forced-tile-mode cases below pin it on the hardware: a
wrong map scatters every output column of the up and the down GEMM.

GEMM cases run through the child of tests/test_gpu_gemm_epilogue.py (and
of tests/test_gpu_gated.py for hidden_act=2): a fresh process per case,
compared against the oracle at the project's bf16 bar (rtol 2e-2,
atol 2e-3 * scale), capacity_factor 2 so nothing is dropped.

The combine cases use capacity_factor 1 at S=128: ONE routing tile, so
which (token, j) slots are dropped is fixed by token order and equals the
oracle's. The dropped counts are pinned, so the kept mask is exercised.
"""
import json
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

from tests import test_gpu_gated as gated
from tests.conftest import REPO_ROOT
from tests.test_gpu_gemm_epilogue import RAGGED, SMALL, run_child

pytestmark = pytest.mark.gpu

CLASSIC = {"FM_FUSED": "0"}


# --- the GEMM epilogues ----------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1, 3, 4])
def test_store16_forced_tile_modes_bf16(mode):
    """RAGGED: partly filled and empty M tiles, a ragged last N tile (the
    per-lane column check of the 16-byte path), 16-byte-aligned rows
    (H=192, P=320 are multiples of 8). PHASE 0 plain and PHASE 1 slots."""
    run_child({"FM_FORCE_MODE": str(mode), **CLASSIC}, **RAGGED)


@pytest.mark.parametrize("mode", [0, 4])
def test_store16_gated_swiglu(mode):
    """hidden_act=2: the 256-wide tile has one output pair per row
    fragment (16 bytes), the 128-wide tile one output (stays 8 bytes)."""
    gated.run_child({"FM_FORCE_MODE": str(mode), **CLASSIC}, **gated.RAGGED)


def test_store16_fp16_mode0():
    run_child({"FM_FORCE_MODE": "0", **CLASSIC}, torch_dtype=3, **RAGGED)


def test_store16_top1_direct_store():
    """top-1: the down epilogue writes moe_out rows directly, unscaled."""
    run_child({"FM_FORCE_MODE": "0", **CLASSIC}, expert_top_k=1, **SMALL)


def test_store16_bias_gelu():
    """Bias and GELU are applied before packing and before the swap."""
    run_child({"FM_FORCE_MODE": "0", **CLASSIC}, bias=True, expert_top_k=2,
              hidden_act=1, **SMALL)


def test_store16_fp8_weights():
    run_child({"FM_FORCE_MODE": "0", **CLASSIC}, expert_top_k=2,
              torch_dtype=4, **SMALL)


def test_store16_persistent_walk_three_forwards():
    """FM_PERSIST_BLOCKS=3: a block's next job starts while the 16-byte
    stores of the previous one are in flight; three forwards, each
    compared."""
    run_child({"FM_FORCE_MODE": "0", "FM_PERSIST_BLOCKS": "3", **CLASSIC},
              runs=3, **RAGGED)


# --- k_cast_combine with dropped slots ---------------------------------------

# Runs in the child. argv[1]: JSON {cfg overrides, dropped}.
COMBINE_CHILD = r"""
import json, sys
import numpy as np
import torch
from oracle.moe_oracle import (OracleConfig, expert_capacity,
                               moe_forward as oracle_forward)
from tests.test_gpu_parity import assert_values, make_cfg
from flashmoe_amd import moe
import flashmoe_amd._ext as _ext

spec = json.loads(sys.argv[1])
cfg, path = make_cfg(**spec["cfg"])
moe.initialize(path, rank=0, world_size=1)
S = cfg["sequence_len"] * cfg["mini_batch"]
H, P, E = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_experts"]
k = cfg["expert_top_k"]
g = torch.Generator(device="cpu").manual_seed(47)
x = torch.randn(1, S, H, generator=g).to(torch.bfloat16).cuda()
gw = torch.randn(H, E, generator=g).to(torch.bfloat16).cuda()
ew = torch.randn(E, 2, P, H, generator=g).to(torch.bfloat16).cuda()
ocfg = OracleConfig(num_experts=E, expert_top_k=k,
                    capacity_factor=cfg["capacity_factor"],
                    drop_tokens=cfg["drop_tokens"],
                    hidden_act=cfg["hidden_act"], element="bf16")
ref = oracle_forward(x.view(S, H).float().cpu().numpy(),
                     gw.float().cpu().numpy().reshape(-1),
                     ew.float().cpu().numpy(), ocfg)
# the oracle's eC are RAW counts (they always sum to S * k); the kept
# slots are those below the capacity
EC = expert_capacity(S, ocfg)
kept = int(np.minimum(ref["eC"], EC).sum())
print("dropped slots:", S * k - kept)
assert kept < S * k, "nothing dropped: the kept mask is not exercised"
assert S * k - kept == spec["dropped"]
out = moe.moe_forward(x, gw, ew)
torch.cuda.synchronize()
assert _ext.load().fm_last_forward_fused() == 0, "fused path ran"
assert_values(out.view(S, H), ref["moe_out"], "bf16", "moe_out",
              rtol=2e-2, atol_scale=2e-3)
moe.finalize()
print("CHILD OK")
"""


def run_combine_child(dropped, **cfg):
    env = dict(os.environ, PYTHONPATH=REPO_ROOT)
    for k in ("FM_FORCE_MODE", "FM_PERSIST_BLOCKS", "FM_PERSIST", "FM_FUSED"):
        env.pop(k, None)
    env.update(CLASSIC)
    spec = {"cfg": cfg, "dropped": dropped}
    r = subprocess.run([sys.executable, "-c", COMBINE_CHILD, json.dumps(spec)],
                       capture_output=True, text=True, timeout=300,
                       cwd=REPO_ROOT, env=env)
    sys.stdout.write(r.stdout[-1500:])
    sys.stderr.write(r.stderr[-3000:])
    assert r.returncode == 0, f"child failed (rc {r.returncode})"
    assert "CHILD OK" in r.stdout


# H / 8 chunks per token against the block's 256 threads: 8 (32 tokens per
# iteration), 24 (10 tokens, 16 threads idle: 256 % 24 != 0), 512 (one
# token per iteration, threads striding: the path for H / 8 >= 256)
@pytest.mark.parametrize("H,dropped", [(64, 13), (192, 9), (4096, 13)])
def test_combine_dropped_slots_top2(H, dropped):
    run_combine_child(dropped, sequence_len=128, num_experts=4,
                      expert_top_k=2, capacity_factor=1, hidden_size=H,
                      intermediate_size=128)


def test_combine_dropped_slots_top3():
    """The flagship's H (two tokens per block iteration) with three slots."""
    run_combine_child(22, sequence_len=128, num_experts=8, expert_top_k=3,
                      capacity_factor=1, hidden_size=1024,
                      intermediate_size=64)
