"""GPU parity tests: the HIP path vs the CPU oracle through the C-ABI.

Bit-exact bar for routing (top-k indices, counts; near-tie escape below),
rtol 2e-2 / atol 2e-3 for bf16 values, 1e-5 fp32.

Determinism note (mirrors the reference, gate.cuh:688-716): inter-tile
order in an expert's token list comes from atomicAdd, so when an expert
OVERFLOWS capacity the kept-token SET is schedule-dependent — in the
reference too. Exact-output tests therefore use either one 128-token tile
(deterministic) or capacity that cannot overflow; full-size runs check
invariants and a capacity-safe configuration. Values under multi-tile
overflow are checked in test_gpu_loads.py, against a reference conditioned
on the kernel's own kept set.
"""
import ctypes
import json
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle.moe_oracle import OracleConfig, moe_forward as oracle_forward

pytestmark = pytest.mark.gpu


def make_cfg(**kw):
    cfg = {
        "capacity_factor": 1, "drop_tokens": 1, "expert_top_k": 2,
        "global_batch": 256, "is_training": 0, "hidden_act": 0,
        "hidden_size": 128, "intermediate_size": 256, "mini_batch": 1,
        "moe_frequency": 1, "num_experts": 8, "num_layers": 1,
        "sequence_len": 128, "torch_dtype": 2, "vocab_size": 32000,
    }
    cfg.update(kw)
    f = tempfile.NamedTemporaryFile("w", suffix=".json", delete=False)
    json.dump(cfg, f)
    f.close()
    return cfg, f.name


@pytest.fixture
def fresh_moe():
    from flashmoe_amd import moe

    yield moe
    try:
        moe.finalize()
    except Exception:
        pass


def run_pair(moe, cfg, cfg_path, seed=47):
    """Run HIP moe_forward and the oracle on identical inputs."""
    from flashmoe_amd.config import torch_dtype_of, weight_dtype_of

    moe.initialize(cfg_path, rank=0, world_size=1)
    S = cfg["sequence_len"] * cfg["mini_batch"]
    H, P, E = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_experts"]
    dt = torch_dtype_of(cfg["torch_dtype"])
    wdt = weight_dtype_of(cfg["torch_dtype"])
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(cfg["mini_batch"], cfg["sequence_len"], H, generator=g).to(dt).cuda()
    gw = torch.randn(H, E, generator=g).to(dt).cuda()
    # dtype 4: weights quantized to fp8e4m3; .float() below dequantizes
    # EXACTLY (every e4m3 value is representable in fp32), so the oracle
    # computes on the same effective weights and the bf16 bar applies
    ew = torch.randn(E, 2, P, H, generator=g).to(wdt).cuda()
    out = moe.moe_forward(x, gw, ew)
    gate_out = moe.gate_output().clone()
    torch.cuda.synchronize()

    element = {0: "fp32", 1: "fp32", 2: "bf16", 3: "fp16", 4: "bf16",
               5: "bf16"}[cfg["torch_dtype"]]
    ocfg = OracleConfig(
        num_experts=E, expert_top_k=cfg["expert_top_k"],
        capacity_factor=cfg["capacity_factor"], drop_tokens=cfg["drop_tokens"],
        hidden_act=cfg["hidden_act"], element=element,
        mx_fp8=(cfg["torch_dtype"] == 5),
    )
    ref = oracle_forward(
        x.view(S, H).float().cpu().numpy(),
        gw.float().cpu().numpy().reshape(-1),
        ew.float().cpu().numpy(),
        ocfg,
    )
    return out.view(S, H), gate_out, ref, ocfg


def assert_values(got_t, want_np, element, what, rtol=None, atol_scale=None):
    got = got_t.float().cpu().numpy()
    scale = max(1.0, float(np.abs(want_np).max()))
    if element == "bf16":
        rtol = rtol or 2e-2
        atol = (atol_scale or 2e-3) * scale
    else:
        rtol = rtol or 1e-5
        atol = (atol_scale or 1e-5) * scale
    ok = np.isclose(got, want_np, rtol=rtol, atol=atol)
    frac = 1.0 - ok.mean()
    assert ok.all(), (
        f"{what}: {100*frac:.3f}% mismatched, max abs err "
        f"{np.abs(got-want_np).max():.5f} (scale {scale:.2f})"
    )


def routing_from_lib(E, EC):
    """Read the kernel's routing via fm_read_routing."""
    import flashmoe_amd._ext as _ext

    lib = _ext.load()
    counts = np.zeros(E, dtype=np.uint32)
    tok = np.zeros(E * EC, dtype=np.uint32)
    ps = np.zeros(E * EC, dtype=np.float32)
    _ext.check(lib.fm_read_routing(
        None,
        ctypes.c_void_p(counts.ctypes.data),
        ctypes.c_void_p(tok.ctypes.data),
        ctypes.c_void_p(ps.ctypes.data)), "fm_read_routing")
    return counts, tok.reshape(E, EC), ps.reshape(E, EC)


# ---------------------------------------------------------------------------


def test_mfma_layout_probe():
    """Verify the assumed mfma_f32_16x16x32_bf16 operand/result layout
    with an asymmetric product (guide par.3: always asymmetric B)."""
    import __graft_entry__  # noqa: F401  (path setup)
    import flashmoe_amd._ext as _ext

    lib = _ext.load()
    g = torch.Generator().manual_seed(0)
    A = torch.randn(16, 32, generator=g).to(torch.bfloat16).cuda()
    Bt = torch.randn(16, 32, generator=g).to(torch.bfloat16).cuda()  # [col][k]
    D = torch.zeros(16, 16, dtype=torch.float32, device="cuda")
    _ext.check(lib.fm_debug_mfma(
        None, ctypes.c_void_p(A.data_ptr()), ctypes.c_void_p(Bt.data_ptr()),
        ctypes.c_void_p(D.data_ptr())), "fm_debug_mfma")
    torch.cuda.synchronize()
    want = A.float() @ Bt.float().T
    assert torch.allclose(D, want, rtol=1e-2, atol=1e-2), (
        f"MFMA layout mismatch: max err {(D-want).abs().max().item()}"
    )


def test_single_tile_bf16_top2(fresh_moe):
    cfg, path = make_cfg()
    out, gate_out, ref, ocfg = run_pair(fresh_moe, cfg, path)
    # routing bit-exact (single tile -> deterministic even with drop)
    E, EC = 8, 32
    counts, tok, ps = routing_from_lib(E, EC)
    clipped = np.minimum(ref["eC"], EC)
    assert np.array_equal(counts.astype(np.int64), clipped)
    for e in range(E):
        assert np.array_equal(tok[e, : counts[e]].astype(np.int64),
                              ref["token_lists"][e]), f"expert {e} token list"
    assert_values(gate_out, ref["gate_out"], "bf16", "gate_out")
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_single_tile_fp32_top1_config1(fresh_moe):
    # BASELINE config 1: 4 experts top-1, seq=128, H=512, P=2048, fp32
    cfg, path = make_cfg(num_experts=4, expert_top_k=1, hidden_size=512,
                         intermediate_size=2048, torch_dtype=0)
    out, gate_out, ref, ocfg = run_pair(fresh_moe, cfg, path)
    assert_values(gate_out, ref["gate_out"], "fp32", "gate_out")
    assert_values(out, ref["moe_out"], "fp32", "moe_out")


def test_single_tile_bf16_top1(fresh_moe):
    """k==1: unscaled direct store path (CombineMode::single,
    processor.cuh:173-204)."""
    cfg, path = make_cfg(expert_top_k=1)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_single_expert_dense_fallback(fresh_moe):
    """E == 1: the reference's dense-FFN fallback shape (moe.cuh:174-177,
    fffn.cuh) — here the generic path routes every token to expert 0."""
    cfg, path = make_cfg(num_experts=1, expert_top_k=1, drop_tokens=0)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    g = gate_out.float().cpu().numpy()
    assert np.allclose(g[:, 0], 1.0, atol=1e-3)  # softmax over one expert
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_single_tile_fp16_top2(fresh_moe):
    """torch_dtype 3 (fp16 element; mfma_f32_16x16x32_f16 path)."""
    cfg, path = make_cfg(torch_dtype=3)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    got = out.float().cpu().numpy()
    scale = max(1.0, float(np.abs(ref["moe_out"]).max()))
    assert np.allclose(got, ref["moe_out"], rtol=2e-2, atol=2e-3 * scale)


def test_multi_tile_fp16_big_kernel(fresh_moe):
    """fp16 through the 256-row kernel (S=2048 -> pEC >= 256), CF=2 so
    capacity cannot overflow (deterministic routing)."""
    cfg, path = make_cfg(torch_dtype=3, sequence_len=2048, capacity_factor=2,
                         hidden_size=256, intermediate_size=512)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    got = out.float().cpu().numpy()
    scale = max(1.0, float(np.abs(ref["moe_out"]).max()))
    assert np.allclose(got, ref["moe_out"], rtol=2e-2, atol=2e-3 * scale)


def test_single_tile_fp8_weights(fresh_moe):
    """torch_dtype 4 (extension): fp8e4m3 expert weights, bf16
    activations/accumulate — the config-5 dtype regime. B is staged as
    raw fp8 through glds and dequantized at fragment read (W8A16)."""
    cfg, path = make_cfg(torch_dtype=4)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    assert_values(gate_out, ref["gate_out"], "bf16", "gate_out")
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_multi_tile_fp8_big_kernel(fresh_moe):
    """fp8 weights through the pipelined big kernel (S=2048, CF=2
    overflow-free -> deterministic routing)."""
    cfg, path = make_cfg(torch_dtype=4, sequence_len=2048, capacity_factor=2,
                         hidden_size=256, intermediate_size=512)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_graph_replay_across_input_changes(fresh_moe):
    """fm_moe_forward captures/replays a hipGraph keyed on the pointer
    tuple; successive calls with DIFFERENT tensors (new allocations) and
    then the ORIGINAL tensors again must each compute on the right data
    (guards against stale-capture bugs)."""
    cfg, path = make_cfg()
    fresh_moe.initialize(path, rank=0, world_size=1)
    from flashmoe_amd.config import torch_dtype_of

    S, H, P, E = 128, 128, 256, 8
    dt = torch_dtype_of(2)
    outs = {}
    tensors = {}
    for tag, seed in (("a", 7), ("b", 1234)):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(1, S, H, generator=g).to(dt).cuda()
        gw = torch.randn(H, E, generator=g).to(dt).cuda()
        ew = torch.randn(E, 2, P, H, generator=g).to(dt).cuda()
        tensors[tag] = (x, gw, ew)
    # a, b, a again (replay of the first graph), repeat b
    for tag in ("a", "b", "a", "b"):
        x, gw, ew = tensors[tag]
        out = fresh_moe.moe_forward(x, gw, ew).clone()
        torch.cuda.synchronize()
        if tag in outs:
            assert torch.equal(out, outs[tag]), f"replay of {tag} diverged"
        else:
            outs[tag] = out
            ocfg = OracleConfig(num_experts=E, expert_top_k=2, element="bf16")
            ref = oracle_forward(x.view(S, H).float().cpu().numpy(),
                                 gw.float().cpu().numpy().reshape(-1),
                                 ew.float().cpu().numpy(), ocfg)
            assert_values(out.view(S, H), ref["moe_out"], "bf16",
                          f"moe_out[{tag}]")


def test_moe_forward_with_biases(fresh_moe):
    """Per-expert bias slabs b_up [E,P] / b_dn [E,H] through the C-ABI
    (the reference's Python API zero-fills biases, python_bindings.cu:80-82,
    but the slabs exist per expert; the C-ABI exposes them)."""
    import flashmoe_amd._ext as _ext
    from flashmoe_amd.config import torch_dtype_of

    cfg, path = make_cfg()
    fresh_moe.initialize(path, rank=0, world_size=1)
    S, H, P, E = 128, 128, 256, 8
    dt = torch_dtype_of(2)
    g = torch.Generator().manual_seed(321)
    x = torch.randn(S, H, generator=g).to(dt).cuda()
    gw = torch.randn(H, E, generator=g).to(dt).cuda()
    ew = torch.randn(E, 2, P, H, generator=g).to(dt).cuda()
    b_up = torch.randn(E, P, generator=g).to(dt).cuda()
    b_dn = torch.randn(E, H, generator=g).to(dt).cuda()
    out = torch.empty(S, H, dtype=dt, device="cuda")
    gate_out = fresh_moe.gate_output()
    lib = _ext.load()
    st = torch.cuda.current_stream().cuda_stream
    _ext.check(lib.fm_moe_forward(
        ctypes.c_void_p(st), ctypes.c_void_p(x.data_ptr()),
        ctypes.c_void_p(gw.data_ptr()), ctypes.c_void_p(ew.data_ptr()),
        ctypes.c_void_p(b_up.data_ptr()), ctypes.c_void_p(b_dn.data_ptr()),
        ctypes.c_void_p(gate_out.data_ptr()), ctypes.c_void_p(out.data_ptr()),
        S), "fm_moe_forward")
    torch.cuda.synchronize()
    ocfg = OracleConfig(num_experts=E, expert_top_k=2, element="bf16")
    ref = oracle_forward(x.float().cpu().numpy(),
                         gw.float().cpu().numpy().reshape(-1),
                         ew.float().cpu().numpy(), ocfg,
                         b_up=b_up.float().cpu().numpy(),
                         b_dn=b_dn.float().cpu().numpy())
    assert_values(out, ref["moe_out"], "bf16", "moe_out(bias)")


def test_expert_ffn_with_bias(fresh_moe):
    """Packed-rows FFN (fm_expert_ffn) with the expert's own bias slab
    (single-expert path: caller passes the slab directly)."""
    import flashmoe_amd._ext as _ext
    from oracle.moe_oracle import expert_ffn as oracle_ffn

    cfg, path = make_cfg()
    fresh_moe.initialize(path, rank=0, world_size=1)
    H, P = 128, 256
    g = torch.Generator().manual_seed(99)
    rows = torch.randn(64, H, generator=g).to(torch.bfloat16).cuda()
    ew = torch.randn(8, 2, P, H, generator=g).to(torch.bfloat16).cuda()
    b_up = torch.randn(P, generator=g).to(torch.bfloat16).cuda()
    b_dn = torch.randn(H, generator=g).to(torch.bfloat16).cuda()
    out = torch.empty_like(rows)
    lib = _ext.load()
    st = torch.cuda.current_stream().cuda_stream
    _ext.check(lib.fm_expert_ffn(
        ctypes.c_void_p(st), ctypes.c_void_p(rows.data_ptr()),
        ctypes.c_void_p(ew.data_ptr()), ctypes.c_void_p(b_up.data_ptr()),
        ctypes.c_void_p(b_dn.data_ptr()), ctypes.c_void_p(out.data_ptr()),
        64, 3), "ffn")
    torch.cuda.synchronize()
    ocfg = OracleConfig(num_experts=8, expert_top_k=2, element="bf16")
    want = oracle_ffn(rows.float().cpu().numpy(),
                      ew[3, 0].float().cpu().numpy(),
                      ew[3, 1].float().cpu().numpy().reshape(-1),
                      b_up.float().cpu().numpy(), b_dn.float().cpu().numpy(),
                      ocfg)
    assert_values(out, want, "bf16", "expert_ffn(bias)")


def test_odd64_shapes_bf16(fresh_moe):
    """H, P multiples of 64 (not 128): the schema's contract; the tile
    guards (B-row clamp + col < N epilogue mask) must handle the ragged
    N tiles (round-1 rejected these shapes)."""
    # capacity_factor 2: EC at CF=1 equals the mean load, so experts
    # overflow and the kept-set becomes schedule-dependent (flaky vs the
    # oracle); headroom keeps the comparison deterministic
    cfg, path = make_cfg(hidden_size=192, intermediate_size=320,
                         sequence_len=256, capacity_factor=2)
    out, gate_out, ref, ocfg = run_pair(fresh_moe, cfg, path)
    assert_values(gate_out, ref["gate_out"], "bf16", "gate_out")
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_odd64_shapes_multi_tile_fp16(fresh_moe):
    # capacity_factor 4: EC=256 leaves headroom so no expert overflows
    # (an overflowing kept-set is schedule-dependent, the documented
    # carve-out); fp16 values at the bf16 tolerance bar - the fp32
    # logits differ from the oracle by MFMA summation order, which flips
    # ~1-ulp of a handful of fp16 softmax probs
    cfg, path = make_cfg(hidden_size=448, intermediate_size=576,
                         sequence_len=512, num_experts=16, torch_dtype=3,
                         capacity_factor=4)
    out, gate_out, ref, ocfg = run_pair(fresh_moe, cfg, path)
    assert_values(gate_out, ref["gate_out"], "fp16", "gate_out",
                  rtol=2e-2, atol_scale=2e-3)
    assert_values(out, ref["moe_out"], "fp16", "moe_out",
                  rtol=2e-2, atol_scale=2e-3)


def test_single_tile_gelu(fresh_moe):
    cfg, path = make_cfg(hidden_act=1)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_single_tile_top4(fresh_moe):
    cfg, path = make_cfg(expert_top_k=4, num_experts=16)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_mini_batch_2(fresh_moe):
    """mini_batch > 1: input [b, s, H] with S = b*s (python_bindings.cu
    validates batch*seq == compiled S; tokens are row-major across the
    batch)."""
    cfg, path = make_cfg(mini_batch=2, sequence_len=128, capacity_factor=2)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    assert out.shape[0] == 256
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


@pytest.mark.parametrize("k", [3, 5, 7])
def test_single_tile_odd_topk(fresh_moe, k):
    """Non-power-of-two top-k (the reference schema allows any k >= 1)."""
    cfg, path = make_cfg(expert_top_k=k, num_experts=16, capacity_factor=2)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


@pytest.mark.parametrize("E,k", [(192, 2), (256, 4)])
def test_many_experts_gate(fresh_moe, E, k):
    """E > 128 (config-5 shape): the expert-chunked gate logits kernel
    and >=192-way top-k routing."""
    # single 128-token tile: routing deterministic even if an expert
    # overflows its tiny capacity (EC = ceil(128/E)*CF*k)
    cfg, path = make_cfg(num_experts=E, expert_top_k=k, sequence_len=128,
                         capacity_factor=2)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    assert_values(gate_out, ref["gate_out"], "bf16", "gate_out")
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_multi_tile_no_overflow_bf16(fresh_moe):
    """Multi-tile S with capacity_factor 2 (overflow-free): exact output
    parity across the nondeterministic tile order."""
    cfg, path = make_cfg(sequence_len=1024, capacity_factor=2,
                         hidden_size=256, intermediate_size=512)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    S, E = 1024, 8
    EC = (S // E) * 2 * 2  # ceil(S/E)*CF*k = 512
    counts, _, _ = routing_from_lib(E, EC)
    assert counts.astype(np.int64).sum() == ref["eC"].sum() == S * 2
    assert np.array_equal(np.sort(counts.astype(np.int64)), np.sort(ref["eC"]))
    assert_values(gate_out, ref["gate_out"], "bf16", "gate_out")
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_training_aux_loss(fresh_moe):
    """is_training=1: gML (mean gate prob) and gMeC (routed fraction)
    accumulators vs the oracle (gate.cuh:273-299,763-773)."""
    from oracle.moe_oracle import gate_aux_loss
    import flashmoe_amd._ext as _ext

    cfg, path = make_cfg(is_training=1, sequence_len=512)
    out, gate_out, ref, ocfg = run_pair(fresh_moe, cfg, path)
    E = cfg["num_experts"]
    lib = _ext.load()
    gML = np.zeros(E, dtype=np.float32)
    gMeC = np.zeros(E, dtype=np.float32)
    _ext.check(lib.fm_read_aux_loss(
        None, ctypes.c_void_p(gML.ctypes.data),
        ctypes.c_void_p(gMeC.ctypes.data)), "aux_loss")
    # oracle reference on the same inputs
    S, H = 512, cfg["hidden_size"]
    g = torch.Generator(device="cpu").manual_seed(47)
    x = torch.randn(1, 512, H, generator=g).to(torch.bfloat16)
    gw = torch.randn(H, E, generator=g).to(torch.bfloat16)
    want_gML, want_gMeC = gate_aux_loss(
        x.view(S, H).float().numpy(),
        gw.float().numpy().reshape(-1).reshape(E, H), ocfg)
    np.testing.assert_allclose(gML, want_gML, rtol=1e-2, atol=1e-4)
    np.testing.assert_allclose(gMeC, want_gMeC, rtol=1e-5, atol=1e-6)


def test_full_bench_size_exact_no_overflow(fresh_moe):
    """Exact value parity at the FULL bench size (S=4096, H=1024, P=4096,
    E=8, k=2) with capacity_factor 2, where no expert can overflow -> the
    kept set is deterministic and the whole [4096, 1024] output must meet
    the tolerance bar vs the oracle (the strongest full-size guarantee the
    routing nondeterminism permits)."""
    cfg, path = make_cfg(sequence_len=4096, hidden_size=1024,
                         intermediate_size=4096, capacity_factor=2)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    assert int(ref["eC"].sum()) == 4096 * 2  # nothing dropped
    assert_values(gate_out, ref["gate_out"], "bf16", "gate_out")
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_bench_config_invariants(fresh_moe):
    """BASELINE config 2 at full size (S=4096, H=1024, P=4096, E=8, k=2,
    CF=1): size-independent properties + routing counts vs oracle
    (kept SETS under overflow are schedule-dependent, as in the
    reference — checked via counts, probs, and finiteness)."""
    cfg, path = make_cfg(sequence_len=4096, hidden_size=1024,
                         intermediate_size=4096)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    S, E, EC = 4096, 8, 1024
    counts, tok, ps = routing_from_lib(E, EC)
    # raw eC is deterministic -> clipped counts match the oracle's
    assert np.array_equal(counts.astype(np.int64), np.minimum(ref["eC"], EC))
    # gate probabilities are schedule-independent
    assert_values(gate_out, ref["gate_out"], "bf16", "gate_out")
    g = gate_out.float().cpu().numpy()
    np.testing.assert_allclose(g[:, :E].sum(1), 1.0, atol=2e-2)
    assert np.isfinite(out.float().cpu().numpy()).all()
    # each kernel-kept (token, expert) slot carries the oracle's mCw
    mcw = ref["mCw"]
    for e in range(E):
        sl = slice(0, counts[e])
        np.testing.assert_allclose(ps[e, sl], mcw[tok[e, sl]], rtol=2e-2)


def test_device_task_queue_probe():
    """Round-2 groundwork: the seqlock MPMC device task ring (subscriber/
    scheduler semantics, os/subscriber.cuh:333-451 / scheduler.cuh:296-441)
    delivers every task exactly once across producer/consumer blocks,
    including ring wrap-around (nTasks >> ring size)."""
    import __graft_entry__  # noqa: F401
    import flashmoe_amd._ext as _ext

    lib = _ext.load()
    n_tasks, ring, blocks = 200_000, 1024, 64
    out = [ctypes.c_uint32() for _ in range(3)]
    _ext.check(lib.fm_debug_taskq(
        None, ring, ctypes.c_longlong(n_tasks), blocks,
        *[ctypes.byref(o) for o in out]), "fm_debug_taskq")
    got_sum, consumed, errors = [int(o.value) for o in out]
    want_sum = sum((s * 2654435761) & 0xFFFFFFFF for s in range(n_tasks)) \
        & 0xFFFFFFFF
    assert errors == 0
    assert consumed == n_tasks
    assert got_sum == want_sum


def test_error_behaviour(fresh_moe):
    """Shape/device validation mirrors the reference's TORCH_CHECKs
    (python_bindings.cu:22-70)."""
    cfg, path = make_cfg()
    fresh_moe.initialize(path, rank=0, world_size=1)
    H, E, P = 128, 8, 256
    x = torch.randn(1, 128, H, dtype=torch.bfloat16, device="cuda")
    gw = torch.randn(H, E, dtype=torch.bfloat16, device="cuda")
    ew = torch.randn(E, 2, P, H, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match="batch\\*seq"):
        fresh_moe.moe_forward(x[:, :64], gw, ew)
    with pytest.raises(ValueError, match="Gate weights"):
        fresh_moe.moe_forward(x, gw.T.contiguous(), ew)
    xx = torch.randn(1, 128, 2 * H, dtype=torch.bfloat16, device="cuda")[..., ::2]
    with pytest.raises(ValueError, match="contiguous"):
        fresh_moe.moe_forward(xx, gw, ew)
    with pytest.raises(ValueError, match="Expert count"):
        fresh_moe.moe_forward(x, gw, ew[:4])


def test_mx_mfma_layout_probe():
    """Pin the empirically determined mfma_scale_f32_16x16x128_f8f6f4
    contract the MX GEMM builds on: lane l holds
    A[row=l&15][k=32*(l>>4)..+32] / B[k-block][col=l&15] as 8 dwords.
    The SCALE byte of lane-group g (opsel-selected, E8M0 = 2^(b-127))
    covers the interleaved 16-element chunk pair
    {k: k>>6 == g&1 and (k>>4)&1 == g>>1} - so supplying the scale of
    CONTIGUOUS 64-block (g&1) on every lane-group scales each hardware
    block uniformly and correctly (what k_quant_mx + the MX GEMM do).
    Wrong lane wiring fails loudly here."""
    import flashmoe_amd._ext as _ext

    lib = _ext.load()
    torch.manual_seed(11)
    A = (torch.randn(16, 128) * 2).to(torch.float8_e4m3fn)
    Bt = (torch.randn(16, 128) * 2).to(torch.float8_e4m3fn)  # [col][k]
    Af, Btf = A.float(), Bt.float()
    rs = np.random.RandomState(3)
    sa64 = rs.randint(125, 130, (16, 2))  # per (row, 64-block)
    sb64 = rs.randint(125, 130, (16, 2))  # per (col, 64-block)
    want = torch.zeros(16, 16)
    for b in range(2):
        blk = Af[:, b * 64:(b + 1) * 64] @ Btf[:, b * 64:(b + 1) * 64].T
        scale = (2.0 ** (torch.tensor(sa64[:, b]).float() - 127)).unsqueeze(1) * \
                (2.0 ** (torch.tensor(sb64[:, b]).float() - 127)).unsqueeze(0)
        want += scale * blk
    # per-lane i32 scale words: lane-group g supplies the contiguous
    # 64-block (g & 1)'s byte (groups 0,2 -> block 0; 1,3 -> block 1)
    saL = np.full(64, 0x7F7F7F7F, dtype=np.uint32)
    sbL = np.full(64, 0x7F7F7F7F, dtype=np.uint32)
    for row in range(16):
        for g in range(4):
            saL[g * 16 + row] = (0x7F7F7F00 | int(sa64[row, g & 1]))
            sbL[g * 16 + row] = (0x7F7F7F00 | int(sb64[row, g & 1]))
    dA = A.cuda().view(torch.uint8).contiguous()
    dB = Bt.cuda().view(torch.uint8).contiguous()
    dsa = torch.from_numpy(saL.view(np.int32).copy()).cuda()
    dsb = torch.from_numpy(sbL.view(np.int32).copy()).cuda()
    D = torch.zeros(16, 16, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _ext.check(lib.fm_debug_mx_mfma(
        ctypes.c_void_p(stream), ctypes.c_void_p(dA.data_ptr()),
        ctypes.c_void_p(dB.data_ptr()), ctypes.c_void_p(dsa.data_ptr()),
        ctypes.c_void_p(dsb.data_ptr()), ctypes.c_void_p(D.data_ptr()), 0),
        "mx_mfma")
    torch.cuda.synchronize()
    got = D.cpu()
    assert torch.allclose(got, want, rtol=1e-3, atol=1e-2), (
        f"MX MFMA layout mismatch: max err {(got-want).abs().max().item()}"
    )


def test_single_tile_mx_fp8(fresh_moe):
    """dtype 5: MX-block-scaled fp8 MFMA - runtime-quantized fp8
    activations (per-64 E8M0 scales) x fp8 weights on
    v_mfma_scale_f32_16x16x128_f8f6f4. The oracle models the e4m3 RNE
    quantization bit-exactly (validated against torch.float8_e4m3fn),
    so the remaining difference is fp32 summation order - the bf16
    tolerance bar applies."""
    cfg, path = make_cfg(torch_dtype=5, intermediate_size=256)
    out, gate_out, ref, ocfg = run_pair(fresh_moe, cfg, path)
    assert_values(gate_out, ref["gate_out"], "bf16", "gate_out")
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_multi_tile_mx_fp8_top4(fresh_moe):
    cfg, path = make_cfg(torch_dtype=5, sequence_len=512, num_experts=16,
                         expert_top_k=4, hidden_size=256,
                         intermediate_size=512, capacity_factor=4)
    out, gate_out, ref, ocfg = run_pair(fresh_moe, cfg, path)
    # rtol 5e-2: the intermediate y is bf16-rounded then re-quantized to
    # e4m3; an MFMA-summation-order flip of one e4m3 rounding step moves
    # the output by ~blockscale * e4m3-ulp (a handful of elements at
    # ~0.5% relative) - inherent to the double-quantized path, not a bug
    assert_values(out, ref["moe_out"], "bf16", "moe_out",
                  rtol=5e-2, atol_scale=5e-3)


def test_mx_fp8_gelu_bias(fresh_moe):
    """dtype 5 with GELU + per-expert bias slabs through the raw ABI."""
    import flashmoe_amd._ext as _ext

    cfg, path = make_cfg(torch_dtype=5, hidden_act=1, sequence_len=256,
                         hidden_size=128, intermediate_size=384,
                         capacity_factor=2)  # no-overflow headroom
    fresh_moe.initialize(path, rank=0, world_size=1)
    lib = _ext.load()
    S, H, P, E = 256, 128, 384, 8
    g = torch.Generator(device="cpu").manual_seed(9)
    x = torch.randn(S, H, generator=g).to(torch.bfloat16).cuda()
    gw = torch.randn(H, E, generator=g).to(torch.bfloat16).cuda()
    ew = torch.randn(E, 2, P, H, generator=g).to(torch.float8_e4m3fn).cuda()
    b_up = torch.randn(E, P, generator=g).to(torch.bfloat16).cuda()
    b_dn = torch.randn(E, H, generator=g).to(torch.bfloat16).cuda()
    gate_out = fresh_moe.gate_output()
    out = torch.empty(S, H, dtype=torch.bfloat16, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _ext.check(lib.fm_moe_forward(
        ctypes.c_void_p(stream), ctypes.c_void_p(x.data_ptr()),
        ctypes.c_void_p(gw.data_ptr()), ctypes.c_void_p(ew.data_ptr()),
        ctypes.c_void_p(b_up.data_ptr()), ctypes.c_void_p(b_dn.data_ptr()),
        ctypes.c_void_p(gate_out.data_ptr()), ctypes.c_void_p(out.data_ptr()),
        S), "fm_moe_forward")
    torch.cuda.synchronize()
    ocfg = OracleConfig(num_experts=E, expert_top_k=2, capacity_factor=2,
                        hidden_act=1, element="bf16", mx_fp8=True)
    ref = oracle_forward(x.float().cpu().numpy(),
                         gw.float().cpu().numpy().reshape(-1),
                         ew.float().cpu().numpy(), ocfg,
                         b_up=b_up.float().cpu().numpy(),
                         b_dn=b_dn.float().cpu().numpy())
    # same double-quantization tolerance note as the top-4 test above
    assert_values(out, ref["moe_out"], "bf16", "moe_out",
                  rtol=5e-2, atol_scale=5e-3)


def _assert_mx_values(out, want):
    """MX double-quantization bar: the intermediate is bf16-rounded then
    e4m3-block-quantized; an fp32-summation-order difference of one
    rounding step moves isolated outputs by ~blockscale * e4m3-ulp
    (~1% of a large value). Require >=99.99% of elements inside the
    rtol 5e-2 bar and NO element beyond 2% of the output scale - a real
    indexing/scale bug fails both (observed failures were 6-99%)."""
    got = out.float().cpu().numpy()
    scale = max(1.0, float(np.abs(want).max()))
    ok = np.isclose(got, want, rtol=5e-2, atol=5e-3 * scale)
    frac_bad = 1.0 - ok.mean()
    max_err = float(np.abs(got - want).max())
    assert frac_bad <= 1e-3 and max_err <= 0.025 * scale, (
        f"moe_out: {100*frac_bad:.4f}% outside tol, max err {max_err:.3f} "
        f"(scale {scale:.1f})")


def test_mx_fp8_mid_geometry_epilogue_quant(fresh_moe):
    """Shapes that engage the MX 128x256 tile WITH in-epilogue
    quantization (jobs >= one wave of CUs): the path the big-shape
    benches run, which the small parity shapes above never reach."""
    cfg, path = make_cfg(torch_dtype=5, sequence_len=2048, num_experts=256,
                         expert_top_k=2, hidden_size=128,
                         intermediate_size=256, capacity_factor=4)
    out, gate_out, ref, ocfg = run_pair(fresh_moe, cfg, path)
    _assert_mx_values(out, ref["moe_out"])


def test_mx_fp8_big_geometry_epilogue_quant(fresh_moe):
    """Shapes that engage the MX 256x256 tile + epilogue quantization
    (M = pEC >= 256 via a high capacity factor)."""
    cfg, path = make_cfg(torch_dtype=5, sequence_len=4096, num_experts=128,
                         expert_top_k=2, hidden_size=128,
                         intermediate_size=256, capacity_factor=8)
    out, gate_out, ref, ocfg = run_pair(fresh_moe, cfg, path)
    _assert_mx_values(out, ref["moe_out"])


@pytest.fixture
def force_fused():
    """Exercise the fused single-launch kernel regardless of the
    shape-keyed default (FM_FUSED is re-read per forward)."""
    os.environ["FM_FUSED"] = "1"
    yield
    os.environ.pop("FM_FUSED", None)


def test_fused_multi_tile_bf16(force_fused, fresh_moe):
    cfg, path = make_cfg(sequence_len=512, num_experts=16, capacity_factor=4)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    assert_values(gate_out, ref["gate_out"], "bf16", "gate_out")
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_fused_top1_fp16(force_fused, fresh_moe):
    cfg, path = make_cfg(torch_dtype=3, expert_top_k=1, sequence_len=256,
                         capacity_factor=2)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    assert_values(out, ref["moe_out"], "fp16", "moe_out",
                  rtol=2e-2, atol_scale=2e-3)


def test_fused_fp8_weights_gelu(force_fused, fresh_moe):
    cfg, path = make_cfg(torch_dtype=4, hidden_act=1, sequence_len=256,
                         capacity_factor=2)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_fused_training_aux(force_fused, fresh_moe):
    import flashmoe_amd._ext as _ext

    cfg, path = make_cfg(is_training=1, sequence_len=256, capacity_factor=2)
    out, gate_out, ref, ocfg = run_pair(fresh_moe, cfg, path)
    lib = _ext.load()
    E = cfg["num_experts"]
    gML = np.zeros(E, dtype=np.float32)
    gMeC = np.zeros(E, dtype=np.float32)
    _ext.check(lib.fm_read_aux_loss(
        None, ctypes.c_void_p(gML.ctypes.data),
        ctypes.c_void_p(gMeC.ctypes.data)), "aux")
    S = 256
    # recompute the aux accumulators from the oracle outputs directly
    probs = ref["gate_out"][:, :E].astype(np.float64)
    want_gML = probs.mean(axis=0)
    sel = ref["topk_idx"]
    want_gMeC = np.bincount(sel.flatten(), minlength=E) / float(S)
    assert np.allclose(gML, want_gML, rtol=2e-2, atol=1e-3)
    assert np.allclose(gMeC, want_gMeC, rtol=1e-6, atol=1e-6)
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_many_experts_512(fresh_moe):
    """E = 512 (the round-2 cap lift; >256 runs the route's 64-token
    half-pass mode with 8 threads/token): single tile, routing bit-exact
    vs the oracle, values at the bf16 bar."""
    cfg, path = make_cfg(num_experts=512, expert_top_k=4, sequence_len=128,
                         hidden_size=128, intermediate_size=128,
                         capacity_factor=2)
    out, gate_out, ref, ocfg = run_pair(fresh_moe, cfg, path)
    E, EC = 512, 2 * 4 * 1  # ceil(128/512)=1, CF=2, k=4
    counts, tok, ps = routing_from_lib(E, EC)
    clipped = np.minimum(ref["eC"], EC)
    assert np.array_equal(counts.astype(np.int64), clipped)
    assert_values(gate_out, ref["gate_out"], "bf16", "gate_out")
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_many_experts_384_multi_tile(fresh_moe):
    cfg, path = make_cfg(num_experts=384, expert_top_k=2, sequence_len=512,
                         hidden_size=128, intermediate_size=128,
                         capacity_factor=8)
    out, gate_out, ref, ocfg = run_pair(fresh_moe, cfg, path)
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_fused_many_experts_384(force_fused, fresh_moe):
    """Fused kernel + E>256 (the route's 64-token half-pass mode runs
    INSIDE k_moe_fused's inline route)."""
    cfg, path = make_cfg(num_experts=384, expert_top_k=2, sequence_len=512,
                         hidden_size=128, intermediate_size=128,
                         capacity_factor=8)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    assert_values(out, ref["moe_out"], "bf16", "moe_out")


def test_fused_odd64_shapes(force_fused, fresh_moe):
    cfg, path = make_cfg(hidden_size=192, intermediate_size=320,
                         sequence_len=256, capacity_factor=2)
    out, gate_out, ref, _ = run_pair(fresh_moe, cfg, path)
    assert_values(out, ref["moe_out"], "bf16", "moe_out")
