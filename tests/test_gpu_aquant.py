"""fp8 activations on torch_dtype 4 (fm_set_activation_quant(1), DESIGN.md
par.5n) on the GPU against tests/aquant_ref.py. Inputs are test_gpu_bscale's
(block scales up to 4x apart); in addition column group j of row r of x is
multiplied by 2^((j + r) % 5 - 2), exact in bf16, so a wrong group or row index
of an activation scale misses by factors (the prescribed-routing case keeps
routing_craft's x: its columns carry the routing). Bar of the forward values:
test_gpu_parity._assert_mx_values (tests/test_aquant_cpu.py shows it holds one
bf16 ulp of the intermediate); each case prints its share inside the bf16 bar.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle.moe_oracle import expert_capacity
from tests.aquant_ref import aquant_moe_forward, make_expert_ffn, quant_g128
from tests.routing_craft import (check_kept, craft_inputs, kept_lists_of,
                                 loads_to_sel)
from tests.test_gpu_bscale import BIG, SHAPES, draw_scales
from tests.test_gpu_parity import (_assert_mx_values, fresh_moe,  # noqa: F401
                                   make_cfg, routing_from_lib)
from tests.test_gpu_wscale import (BF16_BAR, draw, draw_biases, forward_raw,
                                   oracle_cfg)
from tests.test_gpu_wscale import draw_scales as draw_channel_scales

pytestmark = pytest.mark.gpu

FM_ERR_UNSUPPORTED = -4


def lib():
    import flashmoe_amd._ext as _ext
    return _ext.load()


ptr = lambda t: ctypes.c_void_p(t.data_ptr())


def group_factors(x):
    """x with column group j of row r times 2^((j + r) % 5 - 2)."""
    rows = x.reshape(-1, x.shape[-1])
    r = torch.arange(rows.shape[0], device=x.device)[:, None]
    j = torch.arange(rows.shape[1], device=x.device)[None, :] // 128
    return (rows * torch.exp2(((j + r) % 5 - 2).float()).to(x.dtype)).reshape(
        x.shape)


def setup(moe, kw, kind, biased=False):
    """Initialize, draw, attach the weight scales of `kind` ("block",
    "channel" or None)."""
    cfg, path = make_cfg(torch_dtype=4, **kw)
    moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    x = group_factors(x)
    b_up, b_dn = draw_biases(cfg) if biased else (None, None)
    if cfg["hidden_act"] >= 2:
        b_up = None
    if kind == "block":
        sc = draw_scales(cfg)
        moe.set_weight_block_scales(sc)
    elif kind == "channel":
        sc = draw_channel_scales(cfg)
        moe.set_weight_scales(sc)
    else:
        sc = torch.ones_like(draw_channel_scales(cfg))
    return cfg, x, gw, ew, sc, b_up, b_dn


def reference(cfg, x, gw, ew, sc, kind, b_up=None, b_dn=None, quant=True,
              kept=None):
    f = lambda t: t.float().cpu().numpy() if t is not None else None
    S = cfg["sequence_len"] * cfg["mini_batch"]
    return aquant_moe_forward(
        f(x).reshape(S, -1), f(gw).reshape(-1), f(ew), oracle_cfg(cfg), f(sc),
        "block" if kind == "block" else "channel",
        cfg.get("num_shared_experts", 0), f(b_up), f(b_dn), quant, kept)


def check(out, want, what):
    got = out.float().cpu().numpy().reshape(want.shape)
    scale = max(1.0, float(np.abs(want).max()))
    inside = np.isclose(got, want, rtol=BF16_BAR["rtol"],
                        atol=BF16_BAR["atol_scale"] * scale).mean()
    print(f"{what}: {100 * inside:.4f}% inside the bf16 bar")
    _assert_mx_values(out.reshape(want.shape), want)


def run_case(moe, kw, kind="block", biased=True):
    cfg, x, gw, ew, sc, b_up, b_dn = setup(moe, kw, kind, biased)
    moe.set_activation_quant("group128")
    out = forward_raw(moe, cfg, x, gw, ew, b_up, b_dn)
    assert lib().fm_last_forward_fused() == 0
    assert lib().fm_last_forward_decode_ffn() == 0
    S = cfg["sequence_len"] * cfg["mini_batch"]
    assert out.shape == (S, cfg["hidden_size"])
    ref = reference(cfg, x, gw, ew, sc, kind, b_up, b_dn)
    check(out, ref["moe_out"], f"{kw} {kind}")
    return cfg, x, gw, ew, sc, b_up, b_dn, out, ref


def quantiser_rows(rows, K, seed=5):
    """Groups cycle through: amax +448 * 2^k in the first column, -448 * 2^k
    in the last (both with e4m3 ties 17, 19, 2.125 at s = 2^k), a zero group,
    a random group. k in [-29, 6]: |v| from below 2^-20 up to 2^15."""
    g = torch.Generator().manual_seed(seed)
    n = rows * (K // 128)
    v = (torch.randn(n, 128, generator=g) * 50).clamp(-440, 440).bfloat16()
    k = torch.randint(-29, 7, (n, 1), generator=g).float()
    kind = torch.arange(n) % 4
    for f, col, sign in ((0, 0, 1.0), (1, 127, -1.0)):
        v[kind == f, col] = sign * 448.0
        v[kind == f, 5:8] = torch.tensor([17.0, 19.0, 2.125]).bfloat16()
    v[kind == 2] = 0
    return (v.float() * torch.exp2(k)).bfloat16().reshape(rows, K)


@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("rows", [1, 5, 130])
def test_quantiser_bit_for_bit(rows, K):
    a = quantiser_rows(rows, K).cuda()
    q8 = torch.zeros(rows + 1, K, dtype=torch.uint8, device="cuda")
    s = torch.zeros(rows + 1, K // 128, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert lib().fm_quant_fp8_g128(ctypes.c_void_p(st), ptr(a), ptr(q8), ptr(s),
                                   rows, K) == 0
    torch.cuda.synchronize()
    want_q, want_s = quant_g128(a.float().cpu().numpy())
    assert np.array_equal(s[:rows].cpu().numpy().view(np.uint32),
                          want_s.view(np.uint32))
    got_q = q8[:rows].view(torch.float8_e4m3fn).float().cpu().numpy()
    assert np.array_equal(got_q, want_q)
    # exactly `rows` rows are touched
    assert not q8[rows].any() and not s[rows].any()


FORWARD = [(dict(BIG, **s, hidden_act=a), "block") for s in SHAPES
           for a in (0, 2)]
FORWARD += [(dict(BIG, **SHAPES[0], hidden_act=2), "channel"),
            (dict(BIG, **SHAPES[0], hidden_act=2), None),
            (dict(BIG, **SHAPES[0], hidden_act=2, num_shared_experts=1),
             "block"),
            (dict(BIG, **SHAPES[0], hidden_act=2, expert_top_k=1), "block"),
            # the 128x256 down tile: 16 x 1 x 256 jobs fill the chip
            (dict(sequence_len=2048, num_experts=256, expert_top_k=2,
                  capacity_factor=4, hidden_size=256, intermediate_size=128,
                  hidden_act=2), "block")]


@pytest.mark.parametrize("kw,kind", FORWARD)
def test_forward(fresh_moe, kw, kind):
    run_case(fresh_moe, kw, kind)


def test_prescribed_loads(fresh_moe):
    """Loads 0, 1, 129, 126 and 256 (overflowing) at EC = 208; the reference
    is conditioned on the kernel's kept set, as in test_gpu_loads."""
    moe = fresh_moe
    S, E, k, counts = 256, 5, 2, (0, 1, 129, 126, 256)
    cfg, path = make_cfg(torch_dtype=4, sequence_len=S, num_experts=E,
                         expert_top_k=k, capacity_factor=2, hidden_act=2,
                         **SHAPES[0])
    moe.initialize(path, rank=0, world_size=1)
    H = cfg["hidden_size"]
    sel = loads_to_sel(S, E, k, counts, "spread", 7)
    x, gw = craft_inputs(S, H, E, sel, "bf16", 7)
    _, _, ew = draw(cfg)
    sc = draw_scales(cfg)
    moe.set_weight_block_scales(sc)
    moe.set_activation_quant("group128")
    out = moe.moe_forward(x.view(1, S, H).cuda(), gw.cuda(), ew)
    torch.cuda.synchronize()
    EC = expert_capacity(S, oracle_cfg(cfg))
    rc, tok, _ = routing_from_lib(E, EC)
    ref = reference(cfg, x, gw, ew, sc, "block",
                    kept=kept_lists_of(rc, tok))
    assert np.array_equal(ref["topk_idx"], sel)
    check_kept(rc, tok, ref, EC)
    assert rc[4] == EC < counts[4]
    check(out, ref["moe_out"], "prescribed loads")


@pytest.mark.parametrize("S", [5, 127])
def test_decode(fresh_moe, S):
    run_case(fresh_moe, dict(sequence_len=1, mini_batch=S, num_experts=2,
                             expert_top_k=2, drop_tokens=0, hidden_act=2,
                             **SHAPES[0]), biased=False)


def test_expert_ffn_and_segments(fresh_moe):
    """SwiGLU with block scales: fm_expert_ffn on expert 2, two segments
    mapped to experts 3 and 1."""
    cfg, _, _, ew, sc, _, _ = setup(
        fresh_moe, dict(hidden_act=2, num_experts=4, **SHAPES[0]), "block")
    fresh_moe.set_activation_quant("group128")
    g = torch.Generator().manual_seed(99)
    ffn = make_expert_ffn("block")
    ffn_want = lambda cfg, rows, ew, sc, e: ffn(
        rows.float().cpu().numpy(), ew[e].float().cpu().numpy(),
        sc[e].cpu().numpy(), oracle_cfg(cfg))
    H, EC = cfg["hidden_size"], 64  # ceil(128 / 4) * CF 1 * top-2
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = group_factors(torch.randn(130, H, generator=g).bfloat16().cuda())
    out = torch.empty_like(rows)
    assert lib().fm_expert_ffn(st, ptr(rows), ptr(ew), None, None, ptr(out),
                               130, 2) == 0
    torch.cuda.synchronize()
    check(out, ffn_want(cfg, rows, ew, sc, 2), "expert_ffn")
    rows = group_factors(torch.randn(2, EC, H, generator=g).bfloat16().cuda())
    seg = torch.tensor([3, 1], dtype=torch.int32, device="cuda")
    out = torch.empty_like(rows)
    assert lib().fm_expert_ffn_segments(st, ptr(rows), ptr(seg), 2, ptr(ew),
                                        ptr(out)) == 0
    torch.cuda.synchronize()
    for i, e in enumerate((3, 1)):
        check(out[i], ffn_want(cfg, rows[i], ew, sc, e), f"segment {i}")


def test_closer_to_the_quantised_reference_than_quantisation_moves(fresh_moe):
    """rms(got - ref_q) <= 0.25 * rms(ref_q - ref_0) on the first forward
    case; ref_0 is the unquantised bscale_ref forward. e4m3 noise is 2-3 % rms
    per layer, summation order plus the final bf16 rounding 0.1-0.2 %. On the
    CPU rms(ref_q - ref_0) / max|ref_q| is 0.0026 here and 0.0023 for the other
    shape: both under the 1 % at which the other was to be chosen, because the
    group factors give the output heavy tails (max is 14x the rms); against
    rms(ref_q) the quantisation moves the result by 3.7 % and 3.6 %."""
    kw, kind = FORWARD[0]
    cfg, x, gw, ew, sc, b_up, b_dn, out, ref_q = run_case(fresh_moe, kw, kind)
    ref_0 = reference(cfg, x, gw, ew, sc, kind, b_up, b_dn, quant=False)
    rms = lambda a: float(np.sqrt(np.mean(np.square(a, dtype=np.float64))))
    got = out.float().cpu().numpy()
    moved = rms(ref_q["moe_out"] - ref_0["moe_out"])
    err = rms(got - ref_q["moe_out"])
    print(f"rms(got - ref_q) {err:.5f}, rms(ref_q - ref_0) {moved:.5f}, "
          f"moved / max|ref_q| {moved / np.abs(ref_q['moe_out']).max():.5f}")
    assert err <= 0.25 * moved


LIFE = dict(sequence_len=256, num_experts=4, capacity_factor=2, hidden_act=2,
            **SHAPES[0])


def test_lifecycle_and_graph_replay(fresh_moe):
    """Off by default; off after None equals before any set; on differs; on is
    bit-identical eager and through replays (same pointers and stream: the
    forward is captured with the mode off, and the mode is part of the key)."""
    moe = fresh_moe
    cfg, x, gw, ew, sc, _, _ = setup(moe, LIFE, "block")
    assert moe.get_activation_quant() is None
    out = torch.empty(256, cfg["hidden_size"], dtype=torch.bfloat16,
                      device="cuda")
    st = torch.cuda.Stream()
    run = lambda n: [forward_raw(moe, cfg, x, gw, ew, out=out,
                                 stream=st).clone() for _ in range(n)]
    off = run(3)
    moe.set_activation_quant("group128")
    on = run(4)
    assert moe.get_activation_quant() == "group128"
    assert all(torch.equal(o, off[0]) for o in off)
    assert all(torch.equal(o, on[0]) for o in on)
    assert not torch.equal(on[0], off[0])
    check(on[0], reference(cfg, x, gw, ew, sc, "block")["moe_out"], "replay")
    plain = moe.moe_forward(x, gw, ew, activation_quant=None)
    assert torch.equal(plain.reshape(off[0].shape), off[0])
    moe.moe_forward(x, gw, ew, activation_quant="group128")
    moe.finalize()  # finalize and initialize reset the mode
    moe.initialize(make_cfg(torch_dtype=4, **LIFE)[1], rank=0, world_size=1)
    assert lib().fm_get_activation_quant() == 0


@pytest.mark.parametrize("kw,mode,word", [
    (dict(torch_dtype=2), "group128", "torch_dtype"),
    (dict(torch_dtype=5), "group128", "torch_dtype"),
    (dict(torch_dtype=4, hidden_size=192), "group128", "128"),
    (dict(torch_dtype=4, is_training=1), "group128", "is_training"),
    (dict(torch_dtype=4), "group64", "group128"),
])
def test_refusals(fresh_moe, kw, mode, word):
    cfg, path = make_cfg(**kw)
    fresh_moe.initialize(path, rank=0, world_size=1)
    assert lib().fm_set_activation_quant(1 if mode == "group128" else 7) == \
        FM_ERR_UNSUPPORTED
    assert word.encode() in lib().fm_last_error()
    with pytest.raises(ValueError, match=word):
        fresh_moe.set_activation_quant(mode)
    assert lib().fm_get_activation_quant() == 0  # a refused call changes nothing
