"""128x128 block scales of fp8 expert weights (torch_dtype 4,
fm_set_weight_block_scales) on the GPU against tests/bscale_ref.py.

Every block's scale is 2^j * u, j cycling through -2..2 over the flat block
index and u uniform in [1, 1.5) from Generator().manual_seed(48): neighbouring
blocks differ by up to 4x, so a wrong block index, swapped s_glu / s_up, a
transposed down grid or a promotion off by one K tile misses the bar by orders
of magnitude. Weights and inputs are drawn as in test_gpu_wscale.draw. The bar
is the project's bf16 bar with every element inside: rtol 2e-2, atol 2e-3 *
max(1, max|ref|).

FM_FORCE_MODE and FM_FUSED are cached at first use: those cases each run in
one fresh child process.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

from tests.conftest import REPO_ROOT
from tests.bscale_ref import bscale_expert_ffn, bscale_moe_forward
from tests.test_gpu_parity import assert_values, fresh_moe, make_cfg  # noqa: F401
from tests.test_gpu_wscale import (BF16_BAR, draw, draw_biases, env,  # noqa: F401
                                   forward_raw, n_records, oracle_cfg)
from tests.test_gpu_wscale import draw_scales as draw_channel_scales

pytestmark = pytest.mark.gpu

FM_ERR_UNSUPPORTED = -4


def record_len(cfg):
    grid = (cfg["intermediate_size"] // 128) * (cfg["hidden_size"] // 128)
    return (3 if cfg["hidden_act"] >= 2 else 2) * grid


def draw_scales(cfg, seed=48):
    n = n_records(cfg) * record_len(cfg)
    g = torch.Generator(device="cpu").manual_seed(seed)
    u = 1.0 + 0.5 * torch.rand(n, generator=g)
    j = (torch.arange(n) % 5 - 2).float()
    return (torch.exp2(j) * u).reshape(n_records(cfg), -1).cuda()


_REF = {}


def reference(cfg, x, gw, ew, sc, b_up=None, b_dn=None, tag="seed48"):
    """Computed once per (config, scale values) and shared; never modified."""
    key = (json.dumps(cfg, sort_keys=True), tag, b_up is not None)
    if key not in _REF:
        S = cfg["sequence_len"] * cfg["mini_batch"]
        ref = bscale_moe_forward(
            x.reshape(S, -1).float().cpu().numpy(),
            gw.float().cpu().numpy().reshape(-1), ew.float().cpu().numpy(),
            oracle_cfg(cfg), sc.cpu().numpy(),
            cfg.get("num_shared_experts", 0),
            b_up.float().cpu().numpy() if b_up is not None else None,
            b_dn.float().cpu().numpy() if b_dn is not None else None)
        if cfg["capacity_factor"] > 1:  # nothing dropped
            assert int(ref["eC"].sum()) == S * cfg["expert_top_k"]
        _REF[key] = ref["moe_out"]
    return _REF[key]


def check(cfg, out, want, what="moe_out"):
    S = cfg["sequence_len"] * cfg["mini_batch"]
    assert_values(out.reshape(S, -1), want, "bf16", what, **BF16_BAR)


def run_case(moe, kw, biased):
    """One forward with block scales against the reference; relu carries b_up
    and b_dn, a gated act b_dn (raw ABI: moe_forward passes no biases)."""
    cfg, path = make_cfg(torch_dtype=4, **kw)
    moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    sc = draw_scales(cfg)
    b_up, b_dn = draw_biases(cfg) if biased else (None, None)
    if cfg["hidden_act"] >= 2:
        b_up = None
    moe.set_weight_block_scales(sc)
    out = forward_raw(moe, cfg, x, gw, ew, b_up, b_dn)
    check(cfg, out, reference(cfg, x, gw, ew, sc, b_up, b_dn),
          f"moe_out[H {cfg['hidden_size']}, act {cfg['hidden_act']}]")
    return cfg


# --- 1. forward, S >= 128: EC = pEC = 512 rows per expert, no overflow

BIG = dict(sequence_len=512, num_experts=4, expert_top_k=2, capacity_factor=2)
SHAPES = [dict(hidden_size=384, intermediate_size=256),
          dict(hidden_size=256, intermediate_size=384)]
BIG_CASES = [dict(BIG, **s, hidden_act=a) for s in SHAPES for a in (0, 2)]

# Runs in the child. argv[1]: JSON {cfgs: [cfg overrides], fused}.
CHILD = r"""
import json, sys
import torch
from flashmoe_amd import moe
import flashmoe_amd._ext as _ext
from tests.test_gpu_bscale import run_case

spec = json.loads(sys.argv[1])
for kw in spec["cfgs"]:
    run_case(moe, kw, True)
    if spec["fused"]:
        assert _ext.load().fm_last_forward_fused() == 0, "fused path ran"
    moe.finalize()
print("CHILD OK")
"""


def run_child(env_extra, cfgs, fused=False):
    env = dict(os.environ, PYTHONPATH=REPO_ROOT)
    for k in ("FM_FORCE_MODE", "FM_PERSIST_BLOCKS", "FM_PERSIST", "FM_FUSED",
              "FM_DECODE_FFN"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run(
        [sys.executable, "-c", CHILD, json.dumps({"cfgs": cfgs, "fused": fused})],
        capture_output=True, text=True, timeout=300, cwd=REPO_ROOT, env=env)
    sys.stdout.write(r.stdout[-1500:])
    sys.stderr.write(r.stderr[-3000:])
    assert r.returncode == 0, f"child failed (rc {r.returncode})"
    assert "CHILD OK" in r.stdout


@pytest.mark.parametrize("mode", [None, 1, 3, 4, "fused"])
def test_forward_tile_modes(mode):
    """(H, P) = (384, 256) and (256, 384): odd and even K-block counts in both
    GEMMs, several output blocks, 2P = 768 in the gated up phase; relu with
    both biases and SwiGLU with b_dn; the default mode, each forced one, and
    FM_FUSED=1, under which the multi-kernel path must still run."""
    if mode == "fused":
        run_child({"FM_FUSED": "1"}, BIG_CASES[:1], fused=True)
    else:
        run_child({} if mode is None else {"FM_FORCE_MODE": str(mode)},
                  BIG_CASES)


def test_forward_shared_expert(fresh_moe):
    """The shared slices read the last record."""
    run_case(fresh_moe, dict(BIG, **SHAPES[0], hidden_act=2,
                             num_shared_experts=1), True)


# --- 2. decode sizes: E = 2, top-2, every token reaches both experts

@pytest.mark.parametrize("ffn", ["1", "0"])
@pytest.mark.parametrize("S", [4, 33])
def test_decode(fresh_moe, env, S, ffn):
    """33 rows: two row passes of k_decode_ffn. FM_DECODE_FFN=0: the grouped
    GEMMs on the 128x128 tile."""
    import flashmoe_amd._ext as _ext

    env["FM_DECODE_FFN"] = ffn
    run_case(fresh_moe, dict(sequence_len=1, mini_batch=S, num_experts=2,
                             expert_top_k=2, drop_tokens=0, hidden_act=2,
                             **SHAPES[0]), False)
    assert _ext.load().fm_last_forward_decode_ffn() == int(ffn)


# --- 3. fm_expert_ffn: the record of local expert 2, pre-offset

def test_expert_ffn_local_expert_2(fresh_moe):
    import flashmoe_amd._ext as _ext

    cfg, path = make_cfg(torch_dtype=4, hidden_act=2, num_experts=4, **SHAPES[0])
    fresh_moe.initialize(path, rank=0, world_size=1)
    _, _, ew = draw(cfg)
    sc = draw_scales(cfg)
    fresh_moe.set_weight_block_scales(sc)
    g = torch.Generator().manual_seed(99)
    rows = torch.randn(64, cfg["hidden_size"], generator=g).to(
        torch.bfloat16).cuda()
    out = torch.empty_like(rows)
    st = torch.cuda.current_stream().cuda_stream
    _ext.check(_ext.load().fm_expert_ffn(
        ctypes.c_void_p(st), ctypes.c_void_p(rows.data_ptr()),
        ctypes.c_void_p(ew.data_ptr()), None, None,
        ctypes.c_void_p(out.data_ptr()), 64, 2), "fm_expert_ffn")
    torch.cuda.synchronize()
    want = bscale_expert_ffn(rows.float().cpu().numpy(),
                             ew[2].float().cpu().numpy(), sc[2].cpu().numpy(),
                             oracle_cfg(cfg))
    assert_values(out, want, "bf16", "expert_ffn", **BF16_BAR)


# --- 4. lifetime

def granularity():
    import flashmoe_amd._ext as _ext

    ptr, gran = ctypes.c_void_p(), ctypes.c_int32()
    _ext.check(_ext.load().fm_get_weight_scales(
        ctypes.byref(ptr), ctypes.byref(gran)), "fm_get_weight_scales")
    return gran.value, ptr.value or 0


def test_lifetime(fresh_moe):
    moe = fresh_moe
    cfg, path = make_cfg(torch_dtype=4, hidden_act=2, sequence_len=256,
                         num_experts=4, capacity_factor=2, **SHAPES[0])
    moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    assert granularity() == (0, 0)
    plain = moe.moe_forward(x, gw, ew).clone()

    sc = draw_scales(cfg)
    out = moe.moe_forward(x, gw, ew, weight_block_scales=sc)
    torch.cuda.synchronize()
    assert granularity() == (2, sc.data_ptr())
    assert moe.get_weight_scales() is sc
    check(cfg, out, reference(cfg, x, gw, ew, sc), "attached")

    sc.copy_(draw_scales(cfg, seed=49))  # rewritten in place
    out = moe.moe_forward(x, gw, ew)
    torch.cuda.synchronize()
    check(cfg, out, reference(cfg, x, gw, ew, sc, tag="seed49"), "in place")

    moe.set_weight_block_scales(None)
    assert granularity() == (0, 0) and moe.get_weight_scales() is None
    assert torch.equal(moe.moe_forward(x, gw, ew), plain)

    moe.set_weight_block_scales(sc)
    ch = draw_channel_scales(cfg)  # per-channel scales replace block scales
    moe.set_weight_scales(ch)
    assert granularity() == (1, ch.data_ptr())
    per_channel = moe.moe_forward(x, gw, ew).clone()
    moe.set_weight_block_scales(sc)  # and the reverse
    assert granularity() == (2, sc.data_ptr())
    moe.set_weight_scales(ch)
    assert torch.equal(moe.moe_forward(x, gw, ew), per_channel)
    assert not torch.equal(per_channel, plain)


# --- 5. refusals

@pytest.mark.parametrize("kw,word", [
    (dict(torch_dtype=2), "torch_dtype"),
    (dict(torch_dtype=5), "torch_dtype"),
    (dict(torch_dtype=4, hidden_size=192), "128"),
])
def test_refused_configs(fresh_moe, kw, word):
    import flashmoe_amd._ext as _ext

    lib = _ext.load()
    cfg, path = make_cfg(**kw)
    fresh_moe.initialize(path, rank=0, world_size=1)
    sc = torch.ones(cfg["num_experts"], 64, device="cuda")
    rc = lib.fm_set_weight_block_scales(ctypes.c_void_p(sc.data_ptr()))
    assert rc == FM_ERR_UNSUPPORTED
    assert word.encode() in lib.fm_last_error()
    with pytest.raises(ValueError, match=word):
        fresh_moe.set_weight_block_scales(sc)
    assert granularity() == (0, 0)  # refused calls attach nothing
    assert lib.fm_set_weight_block_scales(None) == 0


def test_wrong_tensor(fresh_moe):
    cfg, path = make_cfg(torch_dtype=4, hidden_act=2, **SHAPES[0])
    fresh_moe.initialize(path, rank=0, world_size=1)
    n, BSC = n_records(cfg), record_len(cfg)
    assert BSC == 18
    for bad in (torch.ones(n, BSC - 6, device="cuda"), torch.ones(n, BSC),
                torch.ones(n, BSC, device="cuda", dtype=torch.bfloat16),
                torch.ones(BSC, n, device="cuda").t()):
        with pytest.raises(ValueError, match=rf"\[{n}, {BSC}\]"):
            fresh_moe.set_weight_block_scales(bad)
    assert fresh_moe.get_weight_scales() is None
