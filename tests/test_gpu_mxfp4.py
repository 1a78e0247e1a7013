"""MXFP4 expert weights (torch_dtype 6) on the GPU against the existing
reference forward on tests/mxfp4_ref.dequant's weights with unit scales.
Nibbles uniform over all 16 codes (-0 included), scale bytes uniform in
121..130 (seed 48): neighbouring K blocks and rows differ by factors of 2 to
512, so a wrong row, K block or slab misses by factors and swapped nibbles
miss everywhere. W_eff is exact in bf16, hence the project's bf16 bar.
"""
import ctypes
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.mxfp4_ref import dequant
from tests.test_gpu_aquant import lib, ptr
from tests.test_gpu_bscale import granularity
from tests.test_gpu_parity import assert_values, fresh_moe, make_cfg  # noqa: F401
from tests.test_gpu_wscale import (BF16_BAR, draw, draw_biases, env,  # noqa: F401
                                   forward_raw, n_records, oracle_cfg, record_len)
from tests.wscale_ref import wscale_expert_ffn, wscale_moe_forward

pytestmark = pytest.mark.gpu

FM_ERR_STATE, FM_ERR_UNSUPPORTED = -2, -4
BASE = dict(torch_dtype=6, sequence_len=256, num_experts=4, expert_top_k=2,
            capacity_factor=2, hidden_act=2, hidden_size=256,
            intermediate_size=384)


def draw_mx(cfg, seed=48):
    x, gw, _ = draw(dict(cfg, torch_dtype=2))
    H, P = cfg["hidden_size"], cfg["intermediate_size"]
    mats = 3 if cfg["hidden_act"] >= 2 else 2
    g = torch.Generator(device="cpu").manual_seed(seed)
    ew = torch.randint(0, 256, (n_records(cfg), mats, P, H // 2), generator=g,
                       dtype=torch.uint8)
    sc = torch.randint(121, 131, (n_records(cfg), mats * P * H // 32),
                       generator=g, dtype=torch.uint8)
    return x, gw, ew.cuda(), sc.cuda()


def unit_scales(cfg):
    return np.ones((n_records(cfg), record_len(cfg)), dtype=np.float32)


_REF = {}


def reference(cfg, x, gw, ew, sc, b_up=None, b_dn=None, tag="seed48"):
    key = (json.dumps(cfg, sort_keys=True), tag, b_up is not None)
    if key not in _REF:
        S = cfg["sequence_len"] * cfg["mini_batch"]
        ref = wscale_moe_forward(
            x.reshape(S, -1).float().cpu().numpy(),
            gw.float().cpu().numpy().reshape(-1),
            dequant(ew.cpu().numpy(), sc.cpu().numpy()), oracle_cfg(cfg),
            unit_scales(cfg), cfg.get("num_shared_experts", 0),
            b_up.float().cpu().numpy() if b_up is not None else None,
            b_dn.float().cpu().numpy() if b_dn is not None else None)
        if cfg["capacity_factor"] > 1 or not cfg["drop_tokens"]:
            assert int(ref["eC"].sum()) == S * cfg["expert_top_k"]  # none dropped
        _REF[key] = ref
    return _REF[key]


def run_case(moe, **kw):
    cfg, path = make_cfg(**dict(BASE, **kw))
    moe.initialize(path, rank=0, world_size=1)
    x, gw, ew, sc = draw_mx(cfg)
    b_up, b_dn = draw_biases(cfg)
    if cfg["hidden_act"] >= 2:
        b_up = None
    moe.set_weight_mx_scales(sc)
    out = forward_raw(moe, cfg, x, gw, ew, b_up, b_dn)
    ref = reference(cfg, x, gw, ew, sc, b_up, b_dn)
    assert_values(out, ref["moe_out"], "bf16", f"moe_out{sorted(kw.items())}",
                  **BF16_BAR)
    assert lib().fm_last_forward_fused() == 0
    assert lib().fm_last_forward_decode_ffn() == 0
    return cfg, ref


@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("H,P", [(256, 384), (384, 128)])
def test_forward(fresh_moe, H, P, act):
    """K = 384: three K tiles, scale window moved back; K = 128: one tile."""
    run_case(fresh_moe, hidden_size=H, intermediate_size=P, hidden_act=act)


@pytest.mark.parametrize("kw", [
    dict(expert_top_k=1),
    dict(num_shared_experts=1),
    dict(num_experts=2, drop_tokens=0, capacity_factor=1),
    dict(sequence_len=1, mini_batch=5, drop_tokens=0, capacity_factor=1),
    dict(sequence_len=1, mini_batch=127, drop_tokens=0, capacity_factor=1),
], ids=["top1", "shared", "nodrop_e2", "S5", "S127"])
def test_forward_variants(fresh_moe, env, kw):
    """nodrop_e2: 256 rows per expert. S5 / S127: FM_DECODE_FFN is ignored."""
    if "mini_batch" in kw:
        env["FM_DECODE_FFN"] = "1"
    _, ref = run_case(fresh_moe, **kw)
    if kw.get("num_experts") == 2:
        assert ref["eC"].max() > 128


def test_expert_ffn_entries(fresh_moe):
    """130 rows on local expert 2; two segments mapped to experts 3 and 1."""
    cfg, path = make_cfg(**BASE)
    fresh_moe.initialize(path, rank=0, world_size=1)
    _, _, ew, sc = draw_mx(cfg)
    fresh_moe.set_weight_mx_scales(sc)
    w_eff, ocfg = dequant(ew.cpu().numpy(), sc.cpu().numpy()), oracle_cfg(cfg)
    H, EC = cfg["hidden_size"], 256  # ceil(256 / 4) * CF 2 * top-2
    g = torch.Generator().manual_seed(99)
    rows = torch.randn(2 * EC, H, generator=g).bfloat16().cuda()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def want(lo, hi, e):
        return wscale_expert_ffn(rows[lo:hi].float().cpu().numpy(), w_eff[e],
                                 unit_scales(cfg)[e], ocfg)

    out = torch.zeros_like(rows)
    assert lib().fm_expert_ffn(st, ptr(rows), ptr(ew), None, None, ptr(out),
                               130, 2) == 0, lib().fm_last_error()
    torch.cuda.synchronize()
    assert_values(out[:130], want(0, 130, 2), "bf16", "expert_ffn", **BF16_BAR)
    assert not out[130:].any()  # rows past n_rows are not written

    seg = torch.tensor([3, 1], dtype=torch.int32, device="cuda")
    assert lib().fm_expert_ffn_segments(st, ptr(rows), ptr(seg), 2, ptr(ew),
                                        ptr(out)) == 0, lib().fm_last_error()
    torch.cuda.synchronize()
    for s, e in enumerate((3, 1)):
        assert_values(out[s * EC:(s + 1) * EC], want(s * EC, (s + 1) * EC, e),
                      "bf16", f"ffn_segments[{s}]", **BF16_BAR)


def test_determinism_and_lifecycle(fresh_moe):
    moe = fresh_moe
    cfg, path = make_cfg(**BASE)
    moe.initialize(path, rank=0, world_size=1)
    x, gw, ew, sc = draw_mx(cfg)
    first = moe.moe_forward(x, gw, ew, weight_mx_scales=sc).clone()
    assert granularity() == (3, sc.data_ptr()) and moe.get_weight_scales() is sc
    st = torch.cuda.Stream()
    out = torch.empty_like(first)
    with torch.cuda.stream(st):
        for i in range(4):
            forward_raw(moe, cfg, x, gw, ew, out=out.view(-1, out.size(-1)),
                        stream=st)
            assert torch.equal(out, first), f"forward {i} differs"
        sc[2, 7] += 1  # rewritten in place: expert 2, up row 0, K block 7
        forward_raw(moe, cfg, x, gw, ew, out=out.view(-1, out.size(-1)),
                    stream=st)
    assert not torch.equal(out, first)
    want = reference(cfg, x, gw, ew, sc, tag="bumped")["moe_out"]
    assert_values(out.view(-1, out.size(-1)), want, "bf16", "in place",
                  **BF16_BAR)
    moe.finalize()
    moe.initialize(path, rank=0, world_size=1)
    assert granularity() == (0, 0) and moe.get_weight_scales() is None


@pytest.mark.parametrize("dtype,call,code,word", [
    (4, "mx", FM_ERR_UNSUPPORTED, "torch_dtype"),
    (6, "channel", FM_ERR_UNSUPPORTED, "torch_dtype"),
    (6, "block", FM_ERR_UNSUPPORTED, "torch_dtype"),
    (6, "aquant", FM_ERR_UNSUPPORTED, "torch_dtype"),
    (6, "forward", FM_ERR_STATE, "fm_set_weight_mx_scales"),
])
def test_refusals(fresh_moe, dtype, call, code, word):
    cfg, path = make_cfg(**dict(BASE, torch_dtype=dtype))
    fresh_moe.initialize(path, rank=0, world_size=1)
    buf = torch.full((n_records(cfg), 3 * 384 * 256 // 32), 127,
                     dtype=torch.uint8, device="cuda")
    if call == "forward":
        x, gw, ew, _ = draw_mx(cfg)
        out = torch.full_like(x, 7.0)
        rc = lib().fm_moe_forward(
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ptr(x),
            ptr(gw), ptr(ew), None, None, ptr(fresh_moe.gate_output()),
            ptr(out), 256)
        torch.cuda.synchronize()
        assert (out == 7.0).all()  # nothing ran
    else:
        rc = {"mx": lambda: lib().fm_set_weight_mx_scales(ptr(buf)),
              "channel": lambda: lib().fm_set_weight_scales(ptr(buf), 1),
              "block": lambda: lib().fm_set_weight_block_scales(ptr(buf)),
              "aquant": lambda: lib().fm_set_activation_quant(1)}[call]()
    assert rc == code
    assert word.encode() in lib().fm_last_error()
    assert granularity() == (0, 0) and lib().fm_get_activation_quant() == 0
