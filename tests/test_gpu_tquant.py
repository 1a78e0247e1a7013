"""Per-token fp8 activations on torch_dtype 4 (fm_set_activation_quant(2),
"token") on the GPU against tests/tquant_ref.py. Inputs are
test_gpu_wscale.draw with row r of x times 2^((r % 5) - 2), exact in bf16: a
wrong row or token index of sA misses by factors, and the factor carries into
the intermediate's rows. Bar of the forward values:
test_gpu_parity._assert_mx_values (tests/test_tquant_cpu.py shows it holds one
bf16 ulp of the intermediate)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle.moe_oracle import expert_capacity
from tests.routing_craft import (check_kept, craft_inputs, kept_lists_of,
                                 loads_to_sel)
from tests.test_gpu_aquant import FM_ERR_UNSUPPORTED, lib, ptr, quantiser_rows
from tests.test_gpu_bscale import BIG, SHAPES
from tests.test_gpu_bscale import draw_scales as draw_block_scales
from tests.test_gpu_parity import (_assert_mx_values, fresh_moe,  # noqa: F401
                                   make_cfg, routing_from_lib)
from tests.test_gpu_wscale import (draw, draw_biases, draw_scales, forward_raw,
                                   oracle_cfg)
from tests.tquant_ref import make_expert_ffn, quant_row, tquant_moe_forward

pytestmark = pytest.mark.gpu


def row_factors(x):
    rows = x.reshape(-1, x.shape[-1])
    r = torch.arange(rows.shape[0], device=x.device)[:, None]
    return (rows * torch.exp2((r % 5 - 2).float()).to(x.dtype)).reshape(x.shape)


def setup(moe, kw, scaled=True, biased=False):
    cfg, path = make_cfg(torch_dtype=4, **kw)
    moe.initialize(path, rank=0, world_size=1)
    x, gw, ew = draw(cfg)
    b_up, b_dn = draw_biases(cfg) if biased else (None, None)
    sc = draw_scales(cfg)
    if scaled:
        moe.set_weight_scales(sc)
    return cfg, row_factors(x), gw, ew, sc if scaled else torch.ones_like(sc), \
        b_up, b_dn


def reference(cfg, x, gw, ew, sc, b_up=None, b_dn=None, mode="token",
              kept=None):
    f = lambda t: t.float().cpu().numpy() if t is not None else None
    S = cfg["sequence_len"] * cfg["mini_batch"]
    return tquant_moe_forward(
        f(x).reshape(S, -1), f(gw).reshape(-1), f(ew), oracle_cfg(cfg), f(sc),
        cfg.get("num_shared_experts", 0), f(b_up), f(b_dn), mode,
        kept)["moe_out"]


def run_case(moe, kw, scaled=True):
    cfg, x, gw, ew, sc, b_up, b_dn = setup(moe, kw, scaled,
                                           biased=kw["hidden_act"] < 2)
    moe.set_activation_quant("token")
    out = forward_raw(moe, cfg, x, gw, ew, b_up, b_dn)
    assert lib().fm_last_forward_fused() == 0
    assert lib().fm_last_forward_decode_ffn() == 0
    ref = reference(cfg, x, gw, ew, sc, b_up, b_dn)
    _assert_mx_values(out.reshape(ref.shape), ref)
    return cfg, x, gw, ew, sc, b_up, b_dn, out, ref


# K 128 / 384 / 512: 8 lanes per row; 640: 16; 1152: 32; 2176: 64; 4224: 128
# (two waves); 8320: 256 (four waves); each K but 512 leaves the last chunk
# pass partly idle
@pytest.mark.parametrize("rows,K", [(r, K) for K in (128, 384) for r in
                                    (1, 5, 130)] +
                         [(5, K) for K in (512, 640, 1152, 2176, 4224, 8320)])
def test_quantiser_bit_for_bit(rows, K):
    a = quantiser_rows(rows, K).cuda()
    q8 = torch.zeros(rows + 1, K, dtype=torch.uint8, device="cuda")
    s = torch.zeros(rows + 1, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib().fm_quant_fp8_row(st, ptr(a), ptr(q8), ptr(s), rows, K) == 0
    torch.cuda.synchronize()
    want_q, want_s = quant_row(a.float().cpu().numpy())
    assert np.array_equal(s[:rows].cpu().numpy().view(np.uint32),
                          want_s.view(np.uint32))
    assert np.array_equal(
        q8[:rows].view(torch.float8_e4m3fn).float().cpu().numpy(), want_q)
    assert not q8[rows].any() and not s[rows].any()  # the guard row


def test_quantiser_counted_leaves_rows_past_routed():
    """[3 slices, 40 rows]: counts 0, 7 and 99 under a cap of 33."""
    K, pitch, cap, counts = 640, 40, 33, (0, 7, 99)
    a = quantiser_rows(3 * pitch, K).cuda()
    q8 = torch.full((3 * pitch, K), 0x5A, dtype=torch.uint8, device="cuda")
    s = torch.full((3 * pitch,), -7.0, device="cuda")
    cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib().fm_quant_fp8_row_counted(st, ptr(a), ptr(q8), ptr(s), ptr(cnt),
                                          3, pitch, cap, K) == 0
    torch.cuda.synchronize()
    want_q, want_s = quant_row(a.float().cpu().numpy())
    live = (np.arange(pitch)[None, :] <
            np.minimum(counts, cap)[:, None]).reshape(-1)
    got_q = q8.view(torch.float8_e4m3fn).float().cpu().numpy()
    assert np.array_equal(got_q[live], want_q[live])
    assert np.array_equal(s.cpu().numpy()[live], want_s[live])
    assert (q8.cpu().numpy()[~live] == 0x5A).all()
    assert (s.cpu().numpy()[~live] == -7.0).all()


WIDE = dict(sequence_len=1024, num_experts=256, expert_top_k=2,
            capacity_factor=4, hidden_size=256, intermediate_size=256)
DECODE = dict(sequence_len=1, num_experts=2, expert_top_k=2, drop_tokens=0,
              hidden_act=2, **SHAPES[0])
FORWARD = [(dict(BIG, **s, hidden_act=a), True) for s in SHAPES for a in (0, 2)]
FORWARD += [(dict(BIG, **SHAPES[0], hidden_act=2), False),
            (dict(BIG, **SHAPES[1], hidden_act=0), False),
            (dict(BIG, **SHAPES[0], hidden_act=2, num_shared_experts=1), True),
            (dict(BIG, **SHAPES[0], hidden_act=2, expert_top_k=1), True),
            (dict(DECODE, mini_batch=5), True),
            (dict(DECODE, mini_batch=127), True),
            # 256 jobs of 128x256 fill the chip: the wide tile, up and down
            (dict(WIDE, hidden_act=0), True)]


@pytest.mark.parametrize("kw,scaled", FORWARD)
def test_forward(fresh_moe, kw, scaled):
    run_case(fresh_moe, kw, scaled)


def test_prescribed_loads(fresh_moe):
    """Loads 127, 128, 129, 0, 84 and 300 (overflowing EC = 256); the
    reference is conditioned on the kernel's kept set, as in test_gpu_loads.
    A positive row factor leaves every token's selection as crafted."""
    moe = fresh_moe
    S, E, k, counts = 384, 6, 2, (127, 128, 129, 0, 84, 300)
    cfg, path = make_cfg(torch_dtype=4, sequence_len=S, num_experts=E,
                         expert_top_k=k, capacity_factor=2, hidden_act=2,
                         **SHAPES[0])
    moe.initialize(path, rank=0, world_size=1)
    H = cfg["hidden_size"]
    sel = loads_to_sel(S, E, k, counts, "spread", 7)
    x, gw = craft_inputs(S, H, E, sel, "bf16", 7)
    x = row_factors(x)
    _, _, ew = draw(cfg)
    sc = draw_scales(cfg)
    moe.set_weight_scales(sc)
    moe.set_activation_quant("token")
    out = moe.moe_forward(x.view(1, S, H).cuda(), gw.cuda(), ew)
    torch.cuda.synchronize()
    EC = expert_capacity(S, oracle_cfg(cfg))
    rc, tok, _ = routing_from_lib(E, EC)
    f = lambda t: t.float().cpu().numpy()
    ref = tquant_moe_forward(f(x), f(gw).reshape(-1), f(ew), oracle_cfg(cfg),
                             f(sc), kept_lists=kept_lists_of(rc, tok))
    assert np.array_equal(ref["topk_idx"], sel)
    check_kept(rc, tok, ref, EC)
    assert rc[5] == EC < counts[5]
    _assert_mx_values(out.reshape(S, H), ref["moe_out"])


@pytest.mark.parametrize("entry", ["ffn", "segments", "grouped"])
def test_ep_entry_points(fresh_moe, entry):
    """SwiGLU with per-channel scales: fm_expert_ffn on expert 2, two segments
    mapped to experts 3 and 1, grouped rows of experts 1 and 3."""
    cfg, _, _, ew, sc, _, _ = setup(
        fresh_moe, dict(hidden_act=2, num_experts=4, **SHAPES[0]))
    fresh_moe.set_activation_quant("token")
    g = torch.Generator().manual_seed(99)
    ffn = make_expert_ffn()
    want = lambda rows, e: ffn(
        rows.float().cpu().numpy(), ew[e].float().cpu().numpy(),
        sc[e].cpu().numpy(), oracle_cfg(cfg))
    H, EC = cfg["hidden_size"], 64  # ceil(128 / 4) * CF 1 * top-2
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = 2 * EC if entry == "segments" else 130
    rows = row_factors(torch.randn(n, H, generator=g).bfloat16().cuda())
    out = torch.zeros_like(rows)
    if entry == "ffn":
        parts = [(0, n, 2)]
        rc = lib().fm_expert_ffn(st, ptr(rows), ptr(ew), None, None, ptr(out),
                                 n, 2)
    elif entry == "segments":
        parts = [(0, EC, 3), (EC, n, 1)]
        seg = torch.tensor([3, 1], dtype=torch.int32, device="cuda")
        rc = lib().fm_expert_ffn_segments(st, ptr(rows), ptr(seg), 2, ptr(ew),
                                          ptr(out))
    else:
        parts = [(0, 1, 1), (1, n, 3)]
        offsets = np.array([0, 0, 1, 1, n], dtype=np.int64)
        rc = lib().fm_expert_ffn_grouped(
            st, ptr(rows), ctypes.c_void_p(offsets.ctypes.data), 4, ptr(ew),
            None, None, ptr(out))
    assert rc == 0
    torch.cuda.synchronize()
    for lo, hi, e in parts:
        _assert_mx_values(out[lo:hi], want(rows[lo:hi], e))


@pytest.mark.parametrize("i", [0, 3])
def test_it_is_the_token_semantics(fresh_moe, i):
    """rms(got - ref_token) <= 0.25 * rms(ref_token - ref_other) for the
    group128 and the unquantised reference (test_gpu_aquant's factor).
    Measured ratios: DESIGN.md par.5o."""
    cfg, x, gw, ew, sc, b_up, b_dn, out, ref = run_case(fresh_moe,
                                                        FORWARD[i][0])
    rms = lambda a: float(np.sqrt(np.mean(np.square(a, dtype=np.float64))))
    err = rms(out.float().cpu().numpy().reshape(ref.shape) - ref)
    for mode in ("group128", None):
        moved = rms(ref - reference(cfg, x, gw, ew, sc, b_up, b_dn, mode))
        print(f"{FORWARD[i][0]}: rms(got - ref_token) {err:.5f}, "
              f"rms(ref_token - ref_{mode}) {moved:.5f}, ratio "
              f"{err / moved:.4f}")
        assert err <= 0.25 * moved


LIFE = dict(sequence_len=256, num_experts=4, capacity_factor=2, hidden_act=2,
            **SHAPES[0])


def test_lifecycle_and_graph_replay(fresh_moe):
    """None -> token -> group128 -> None: each mode its own result, each
    bit-identical eager and through replays (same pointers and stream; the
    mode is part of the graph key); finalize / initialize reset the mode."""
    moe = fresh_moe
    cfg, x, gw, ew, sc, _, _ = setup(moe, LIFE)
    out = torch.empty(256, cfg["hidden_size"], dtype=torch.bfloat16,
                      device="cuda")
    st = torch.cuda.Stream()
    got = {}
    for mode in (None, "token", "group128", None):
        moe.set_activation_quant(mode)
        assert moe.get_activation_quant() == mode
        runs = [forward_raw(moe, cfg, x, gw, ew, out=out, stream=st).clone()
                for _ in range(4)]
        assert all(torch.equal(o, runs[0]) for o in runs)
        assert torch.equal(got.setdefault(mode, runs[0]), runs[0])
    assert not torch.equal(got["token"], got[None])
    assert not torch.equal(got["token"], got["group128"])
    ref = reference(cfg, x, gw, ew, sc)
    _assert_mx_values(got["token"].reshape(ref.shape), ref)
    tok = moe.moe_forward(x, gw, ew, activation_quant="token")
    assert torch.equal(tok.reshape(out.shape), got["token"])
    moe.finalize()
    moe.initialize(make_cfg(torch_dtype=4, **LIFE)[1], rank=0, world_size=1)
    assert lib().fm_get_activation_quant() == 0


@pytest.mark.parametrize("kw,word", [
    (dict(torch_dtype=2), "torch_dtype"),
    (dict(torch_dtype=5), "torch_dtype"),
    (dict(torch_dtype=4, hidden_size=192), "128"),
    (dict(torch_dtype=4, is_training=1), "is_training"),
])
def test_refusals(fresh_moe, kw, word):
    cfg, path = make_cfg(**kw)
    fresh_moe.initialize(path, rank=0, world_size=1)
    assert lib().fm_set_activation_quant(2) == FM_ERR_UNSUPPORTED
    assert word.encode() in lib().fm_last_error()
    assert b"token" in lib().fm_last_error()
    with pytest.raises(ValueError, match=word):
        fresh_moe.set_activation_quant("token")
    assert lib().fm_get_activation_quant() == 0  # a refused call changes nothing
    assert lib().fm_set_activation_quant(7) == FM_ERR_UNSUPPORTED
    assert b"group128" in lib().fm_last_error()
    assert b"token" in lib().fm_last_error()


@pytest.mark.parametrize("first", ["block", "token"])
def test_token_and_block_scales_refuse_each_other(fresh_moe, first):
    moe = fresh_moe
    cfg, path = make_cfg(torch_dtype=4, **SHAPES[0])
    moe.initialize(path, rank=0, world_size=1)
    bs = draw_block_scales(cfg)
    gran = ctypes.c_int32(-1)
    if first == "block":
        moe.set_weight_block_scales(bs)
        assert lib().fm_set_activation_quant(2) == FM_ERR_UNSUPPORTED
        with pytest.raises(ValueError, match="block scales"):
            moe.set_activation_quant("token")
        want = (0, 2)
    else:
        moe.set_activation_quant("token")
        assert lib().fm_set_weight_block_scales(ptr(bs)) == FM_ERR_UNSUPPORTED
        with pytest.raises(ValueError, match="token"):
            moe.set_weight_block_scales(bs)
        want = (2, 0)
    err = lib().fm_last_error()
    assert b"token" in err and b"block scales" in err
    lib().fm_get_weight_scales(None, ctypes.byref(gran))
    assert (lib().fm_get_activation_quant(), gran.value) == want
