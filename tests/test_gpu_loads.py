"""Per-expert row counts placed on tile and capacity edges: prescribed
routing (tests/routing_craft.py) on the GPU against the kept-set-conditional
reference.

Every forward here reads the kernel's routing back (fm_read_routing), checks
that the kept set is a legal one for the prescribed selection (check_kept),
and compares gate_out and moe_out with forward_given_kept ON THAT KEPT SET -
so values are checked under capacity overflow with several 128-token tiles
too, where the kept set depends on the block order. Tokens that lost every
slot must come out exactly zero (the shared term alone with shared experts).

Bars are the project's own, unchanged (test_gpu_parity.assert_values: rtol
2e-2, atol 2e-3 * scale for bf16 / fp16 / fp8 weights, 1e-5 for fp32;
_assert_mx_values for dtype 5), every element inside.

Shapes (tests/routing_craft.LOADS; each count vector in a "spread" and a
"blocked" token layout):
  L  S=512, E=4, top-2, no drop (EC = pEC = 2048), H=192, P=320: 0, 1, 127,
     128, 129, 255, 256, 257, 383, 384, 385 and 512 rows per expert - partly
     filled M tiles of the 128- and 256-row tiles in every forced mode, the
     persistent walk and the single-launch kernel.
  O  S=512, E=4, top-2, CF=1 (EC = 256), H=128, P=256: overflow by 256 and by
     one, exactly at capacity, one under; every token on two overflowing
     experts. O8: S=384, E=8, EC = 96 (pEC = 128).
  D  S=96, E=4, top-2, no drop: 31 / 32 / 33 rows around the 32-row passes of
     k_decode_ffn, and S=1, S=5.

FM_FORCE_MODE, FM_PERSIST_BLOCKS and FM_FUSED cases run in one fresh child
process each (the first two are cached at first use); a child initializes
once and runs all load patterns of its shape, only x changes between them.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle.moe_oracle import OracleConfig, _elem_round, expert_capacity
from tests.conftest import REPO_ROOT
from tests.routing_craft import (LOADS, check_kept, craft_inputs,
                                 forward_given_kept, kept_lists_of,
                                 loads_to_sel, patterns, wholly_dropped)
from tests.test_gpu_parity import (_assert_mx_values, assert_values,  # noqa: F401
                                   fresh_moe, make_cfg, routing_from_lib)

pytestmark = pytest.mark.gpu

ELEMENT = {0: "fp32", 2: "bf16", 3: "fp16", 4: "bf16", 5: "bf16"}

L_CFG = dict(drop_tokens=0, capacity_factor=2, hidden_size=192,
             intermediate_size=320)
D_CFG = dict(drop_tokens=0)


def bar(element):
    # assert_values applies its fp32 bar to everything that is not "bf16";
    # fp16 carries the bf16 bar (as in test_gpu_gemm_epilogue)
    return {} if element == "fp32" else dict(rtol=2e-2, atol_scale=2e-3)


def run_loads(moe, name, rounds=1, only=None, want_fused=None,
              want_decode=None, scaled=False, **kw):
    """Initialize once for LOADS[name] under the config overrides kw, then run
    every load pattern (`only`: indices of the count vectors to run), `rounds`
    times over, each forward checked as the module docstring says."""
    import flashmoe_amd._ext as _ext
    from flashmoe_amd.config import (expert_mats, torch_dtype_of,
                                     weight_dtype_of)

    S, E, k = (LOADS[name][key] for key in "SEk")
    kw.update(num_experts=E, expert_top_k=k)
    kw.update(dict(sequence_len=S) if S >= 128 else
              dict(sequence_len=1, mini_batch=S))
    cfg, path = make_cfg(**kw)
    H, P = cfg["hidden_size"], cfg["intermediate_size"]
    nSh = cfg.get("num_shared_experts", 0)
    dtc = cfg["torch_dtype"]
    element = ELEMENT[dtc]
    ocfg = OracleConfig(
        num_experts=E, expert_top_k=k, capacity_factor=cfg["capacity_factor"],
        drop_tokens=cfg["drop_tokens"], hidden_act=cfg["hidden_act"],
        element=element, mx_fp8=(dtc == 5))
    EC = expert_capacity(S, ocfg)

    moe.initialize(path, rank=0, world_size=1)
    lib = _ext.load()
    g = torch.Generator(device="cpu").manual_seed(47)
    ew = torch.randn(E + nSh, expert_mats(cfg["hidden_act"]), P, H,
                     generator=g).to(weight_dtype_of(dtc)).cuda()
    ew_np = ew.float().cpu().numpy()
    sc_np = None
    if scaled:  # exp2(U(-2, 1)) per channel, as in test_gpu_wscale
        u = torch.rand(E + nSh, P + H + (P if cfg["hidden_act"] >= 2 else 0),
                       generator=g)
        sc = torch.exp2(3.0 * u - 2.0).cuda()
        moe.set_weight_scales(sc)
        sc_np = sc.cpu().numpy()

    pats = [p for p in patterns(name)
            if only is None or LOADS[name]["counts"].index(p[0]) in only]
    inputs, refs, gw_dev = {}, {}, None
    for rnd in range(rounds):
        for counts, layout, seed in pats:
            what = f"{name} {counts} {layout} round {rnd}"
            if (counts, layout) not in inputs:
                sel = loads_to_sel(S, E, k, counts, layout, seed)
                x, gw = craft_inputs(S, H, E, sel, element, seed)
                if gw_dev is None:
                    gw_dev, gw_np = gw.cuda(), gw.float().numpy().reshape(-1)
                assert torch.equal(gw, gw_dev.cpu())  # only x changes
                inputs[counts, layout] = (
                    sel, x.float().numpy(),
                    x.view(cfg["mini_batch"], cfg["sequence_len"], H).to(
                        torch_dtype_of(dtc)).cuda())
            sel, x_np, x_dev = inputs[counts, layout]

            out = moe.moe_forward(x_dev, gw_dev, ew)
            gate_out = moe.gate_output()
            torch.cuda.synchronize()
            if want_fused is not None:
                assert lib.fm_last_forward_fused() == want_fused, what
            if want_decode is not None:
                assert lib.fm_last_forward_decode_ffn() == want_decode, what

            rc, tok, _ = routing_from_lib(E, EC)
            kept = kept_lists_of(rc, tok)
            key = (counts, layout, b"".join(l.tobytes() for l in kept),
                   tuple(map(len, kept)))
            if key not in refs:  # computed once per kept set, never modified
                refs[key] = forward_given_kept(
                    x_np, gw_np, ew_np, ocfg, kept, n_shared=nSh, scales=sc_np)
            ref = refs[key]
            assert np.array_equal(ref["topk_idx"], sel), what
            assert np.array_equal(ref["eC"], np.asarray(counts)), what
            check_kept(rc, tok, ref, EC)

            got = out.view(S, H).float().cpu().numpy()
            gone = wholly_dropped(S, kept)
            err = float(np.abs(got - ref["moe_out"]).max())
            print(f"{what}: kept {[len(l) for l in kept]}, wholly dropped "
                  f"{int(gone.sum())}, max abs err {err:.4f} (max |ref| "
                  f"{float(np.abs(ref['moe_out']).max()):.1f})", flush=True)

            assert_values(gate_out, ref["gate_out"], element,
                          f"gate_out[{what}]", **bar(element))
            if dtc == 5:
                _assert_mx_values(out.view(S, H), ref["moe_out"])
            else:
                assert_values(out.view(S, H), ref["moe_out"], element,
                              f"moe_out[{what}]", **bar(element))

            # tokens that lost every slot
            lost_slots = int(np.maximum(np.asarray(counts) - EC, 0).sum())
            if k == 1:
                assert int(gone.sum()) == lost_slots, what
            if lost_slots and set(counts) <= {0, S}:
                # every token selects overflowing experts only
                assert gone.any(), f"{what}: no token lost all of its slots"
            if nSh == 0:
                assert not got[gone].any(), \
                    f"{what}: a wholly dropped token's row is not zero"
            else:  # the shared term alone (within the bar, by the above)
                assert np.array_equal(
                    ref["moe_out"][gone],
                    _elem_round(ref["shared_out"][gone], element)), what
    moe.finalize()


# --- child processes

CHILD = ("import sys; from tests.test_gpu_loads import child_main; "
         "child_main(sys.argv[1])")


def child_main(arg):
    from flashmoe_amd import moe

    for job in json.loads(arg):
        run_loads(moe, **job)
    print("CHILD OK")


def run_child(env_extra, *jobs):
    """One fresh interpreter under env_extra runs the jobs (run_loads keyword
    sets) in turn and stops at the first failure."""
    env = dict(os.environ, PYTHONPATH=REPO_ROOT)
    for key in ("FM_FORCE_MODE", "FM_PERSIST_BLOCKS", "FM_PERSIST", "FM_FUSED",
                "FM_DECODE_FFN", "FM_GATE_FUSED"):
        env.pop(key, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(jobs)],
                       capture_output=True, text=True, timeout=300,
                       cwd=REPO_ROOT, env=env)
    sys.stdout.write(r.stdout[-6000:])
    sys.stderr.write(r.stderr[-3000:])
    assert r.returncode == 0, f"child failed (rc {r.returncode})"
    assert "CHILD OK" in r.stdout


def classic(mode=None, **extra):
    env = {"FM_FUSED": "0", **extra}
    if mode is not None:
        env["FM_FORCE_MODE"] = str(mode)
    return env


# --- shape L: tile edges, nothing dropped

@pytest.mark.parametrize("mode", [0, 1, 3, 4])
def test_tile_edges_forced_mode_bf16(mode):
    run_child(classic(mode), dict(name="L", want_fused=0, **L_CFG))


def test_tile_edges_default_mode_bf16():
    run_child(classic(), dict(name="L", want_fused=0, **L_CFG))


@pytest.mark.parametrize("mode", [0, 4])
def test_tile_edges_persistent_walk_three_blocks(mode):
    """Three blocks walk every job, three forwards per pattern in sequence:
    the walk starts on the empty jobs of an expert without rows, meets partly
    filled tiles between full and empty ones, and carries nothing from one
    pattern to the next."""
    run_child(classic(mode, FM_PERSIST_BLOCKS="3"),
              dict(name="L", rounds=3, want_fused=0, **L_CFG))


def test_tile_edges_fused_kernel():
    """The single-launch kernel (its waits are bounded: a give-up is an error
    of the forward, and fails the child)."""
    run_child({"FM_FUSED": "1"}, dict(name="L", want_fused=1, **L_CFG))


def test_tile_edges_mode0_fp16():
    run_child(classic(0), dict(name="L", torch_dtype=3, **L_CFG))


def test_tile_edges_mode0_fp8_weights():
    run_child(classic(0), dict(name="L", torch_dtype=4, **L_CFG))


def test_tile_edges_mode0_swiglu():
    run_child(classic(0), dict(name="L", hidden_act=2, **L_CFG))


def test_tile_edges_mode4_one_shared_expert():
    run_child(classic(4), dict(name="L", num_shared_experts=1, **L_CFG))


def test_tile_edges_fp32(fresh_moe):
    run_loads(fresh_moe, "L", torch_dtype=0, **L_CFG)


def test_tile_edges_top1(fresh_moe):
    run_loads(fresh_moe, "L_top1", **L_CFG)


def test_tile_edges_top3(fresh_moe):
    run_loads(fresh_moe, "L_top3", **L_CFG)


def test_tile_edges_mx_fp8(fresh_moe):
    """dtype 5: (512, 256, 255, 1) and (512, 512, 0, 0)."""
    run_loads(fresh_moe, "L", only=(0, 3), torch_dtype=5,
              **dict(L_CFG, hidden_size=128, intermediate_size=256))


# --- shape O: capacity edges with drops, several routing tiles

def test_capacity_edges_default_mode_bf16(fresh_moe):
    run_loads(fresh_moe, "O")


@pytest.mark.parametrize("mode", [0, 4])
def test_capacity_edges_forced_mode_bf16(mode):
    run_child(classic(mode), dict(name="O", want_fused=0))


def test_capacity_edges_fused_kernel():
    run_child({"FM_FUSED": "1"}, dict(name="O", want_fused=1))


def test_capacity_edges_swiglu(fresh_moe):
    run_loads(fresh_moe, "O", hidden_act=2)


def test_capacity_edges_one_shared_expert(fresh_moe):
    """A token that lost both routed slots keeps the shared term alone."""
    run_loads(fresh_moe, "O", num_shared_experts=1)


def test_capacity_edges_fp8_weight_scales(fresh_moe):
    run_loads(fresh_moe, "O", torch_dtype=4, scaled=True)


def test_capacity_edges_top1(fresh_moe):
    """top-1 (the direct store): a dropped token's row is exactly zero."""
    run_loads(fresh_moe, "O_top1")


def test_capacity_96_rows_in_a_128_row_tile(fresh_moe):
    """S=384, E=8: EC = 96 is no multiple of the tile, pEC = 128."""
    run_loads(fresh_moe, "O8")


# --- shape D: decode sizes

@pytest.mark.parametrize("ffn", [0, 1])
@pytest.mark.parametrize("dtype_code,act", [(2, 0), (2, 2), (4, 0), (4, 2)])
def test_decode_row_pass_edges(fresh_moe, monkeypatch, dtype_code, act, ffn):
    """FM_DECODE_FFN is re-read per forward: 1 the weight-streaming kernels
    (32 rows per pass), 0 the grouped GEMMs."""
    monkeypatch.setenv("FM_DECODE_FFN", str(ffn))
    run_loads(fresh_moe, "D", want_decode=ffn, want_fused=0,
              torch_dtype=dtype_code, hidden_act=act, **D_CFG)


@pytest.mark.parametrize("ffn", [0, 1])
@pytest.mark.parametrize("dtype_code,act", [(2, 0), (4, 2)])
@pytest.mark.parametrize("name", ["D1", "D5"])
def test_decode_all_tokens_on_two_experts(fresh_moe, monkeypatch, name,
                                          dtype_code, act, ffn):
    monkeypatch.setenv("FM_DECODE_FFN", str(ffn))
    run_loads(fresh_moe, name, want_decode=ffn, want_fused=0,
              torch_dtype=dtype_code, hidden_act=act, **D_CFG)
