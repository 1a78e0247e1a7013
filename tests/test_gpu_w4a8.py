"""fm_set_activation_quant(3), "mxfp8" (DESIGN.md par.5q), on the GPU against
tests/w4a8_ref.py. Inputs: test_gpu_mxfp4.draw_mx with column block c // 32 of
x times 2^((c // 32) % 5 - 2), exact in bf16, so neighbouring activation blocks
carry different scale bytes next to weight scale bytes 121..130: a wrong block,
lane-group, register half or operand pairing misses by factors. Bar:
test_gpu_parity._assert_mx_values (tests/test_w4a8_cpu.py shows it holds)."""
import ctypes
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.mxfp4_ref import dequant as dequant_w
from tests.test_gpu_aquant import FM_ERR_UNSUPPORTED, lib, ptr, quantiser_rows
from tests.test_gpu_mxfp4 import BASE, draw_mx
from tests.test_gpu_parity import (_assert_mx_values, fresh_moe,  # noqa: F401
                                   make_cfg)
from tests.test_gpu_wscale import draw_biases, env, forward_raw, oracle_cfg  # noqa: F401
from tests.w4a8_ref import expert_ffn, quant_mx32, w4a8_moe_forward

pytestmark = pytest.mark.gpu


def block_factors(x):
    c = torch.arange(x.shape[-1], device=x.device) // 32
    return x * torch.exp2((c % 5 - 2).float()).to(x.dtype)


_REF = {}  # computed once per config and shared; never modified


def reference(cfg, x, gw, ew, sc, b_up=None, b_dn=None):
    key = (json.dumps(cfg, sort_keys=True), b_up is not None)
    if key not in _REF:
        f = lambda t: t.float().cpu().numpy() if t is not None else None
        S = cfg["sequence_len"] * cfg["mini_batch"]
        _REF[key] = w4a8_moe_forward(
            f(x).reshape(S, -1), f(gw).reshape(-1),
            dequant_w(ew.cpu().numpy(), sc.cpu().numpy()), oracle_cfg(cfg),
            cfg.get("num_shared_experts", 0), f(b_up), f(b_dn))
    return _REF[key]


def run_case(moe, biased=False, **kw):
    cfg, path = make_cfg(**dict(BASE, **kw))
    moe.initialize(path, rank=0, world_size=1)
    x, gw, ew, sc = draw_mx(cfg)
    x = block_factors(x)
    b_up, b_dn = draw_biases(cfg) if biased else (None, None)
    moe.set_weight_mx_scales(sc)
    moe.set_activation_quant("mxfp8")
    out = forward_raw(moe, cfg, x, gw, ew, b_up, b_dn)
    assert lib().fm_last_forward_fused() == 0
    assert lib().fm_last_forward_decode_ffn() == 0
    ref = reference(cfg, x, gw, ew, sc, b_up, b_dn)
    _assert_mx_values(out, ref["moe_out"])
    return cfg, ref


@pytest.mark.parametrize("rows,K,counts", [(r, K, None) for K in (128, 384)
                                           for r in (1, 5, 130)] +
                         [(5, 640, None), (4100, 1024, None),
                          (120, 384, (0, 7, 99))])
def test_quantiser_bit_for_bit(rows, K, counts):
    """5 x 640: a block partly idle; 4100 x 1024: past one pass of the grid;
    counts: [3, 40] rows under a cap of 33. The guard row and dead rows stay."""
    a = quantiser_rows(rows, K).cuda()
    q8 = torch.full((rows + 1, K), 0x5A, dtype=torch.uint8, device="cuda")
    s = q8[:, :K // 32].clone()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if counts is None:
        rc = lib().fm_quant_mxfp8(st, ptr(a), ptr(q8), ptr(s), rows, K)
        live = np.arange(rows + 1) < rows
    else:
        cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
        rc = lib().fm_quant_mxfp8_counted(st, ptr(a), ptr(q8), ptr(s),
                                          ptr(cnt), 3, 40, 33, K)
        live = np.append(np.arange(40) < np.minimum(counts, 33)[:, None], False)
    assert rc == 0
    torch.cuda.synchronize()
    want_q, want_s = quant_mx32(a.float().cpu().numpy())
    got_q = q8.view(torch.float8_e4m3fn).float().cpu().numpy()
    assert np.array_equal(got_q[live], want_q[live[:-1]])
    assert np.array_equal(s.cpu().numpy()[live], want_s[live[:-1]])
    assert (q8.cpu().numpy()[~live] == 0x5A).all()
    assert (s.cpu().numpy()[~live] == 0x5A).all()


@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("H,P", [(256, 384), (384, 128)])
def test_forward(fresh_moe, H, P, act):
    run_case(fresh_moe, hidden_size=H, intermediate_size=P, hidden_act=act)


@pytest.mark.parametrize("kw", [
    dict(expert_top_k=1),
    dict(num_shared_experts=1),
    dict(num_experts=2, drop_tokens=0, capacity_factor=1),
    dict(sequence_len=1, mini_batch=5, drop_tokens=0, capacity_factor=1),
    dict(sequence_len=1, mini_batch=127, drop_tokens=0, capacity_factor=1),
    dict(hidden_act=1, biased=True),
], ids=["top1", "shared", "nodrop_e2", "S5", "S127", "gelu_biases"])
def test_forward_variants(fresh_moe, env, kw):
    """nodrop_e2: two M tiles per expert. S5 / S127: FM_DECODE_FFN ignored."""
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
    fresh_moe.set_activation_quant("mxfp8")
    w_eff, ocfg = dequant_w(ew.cpu().numpy(), sc.cpu().numpy()), oracle_cfg(cfg)
    H, P, EC = cfg["hidden_size"], cfg["intermediate_size"], 256
    ones = np.ones(2 * P + H, dtype=np.float32)
    g = torch.Generator().manual_seed(99)
    rows = block_factors(torch.randn(2 * EC, H, generator=g).bfloat16().cuda())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    want = lambda lo, hi, e: expert_ffn(rows[lo:hi].float().cpu().numpy(),
                                        w_eff[e], ones, ocfg)
    out = torch.zeros_like(rows)
    assert lib().fm_expert_ffn(st, ptr(rows), ptr(ew), None, None, ptr(out),
                               130, 2) == 0, lib().fm_last_error()
    torch.cuda.synchronize()
    _assert_mx_values(out[:130], want(0, 130, 2))
    assert not out[130:].any()  # rows past n_rows are not written
    seg = torch.tensor([3, 1], dtype=torch.int32, device="cuda")
    assert lib().fm_expert_ffn_segments(st, ptr(rows), ptr(seg), 2, ptr(ew),
                                        ptr(out)) == 0, lib().fm_last_error()
    torch.cuda.synchronize()
    for s, e in enumerate((3, 1)):
        _assert_mx_values(out[s * EC:(s + 1) * EC],
                          want(s * EC, (s + 1) * EC, e))


def test_determinism_and_lifecycle(fresh_moe):
    moe = fresh_moe
    cfg, path = make_cfg(**BASE)
    moe.initialize(path, rank=0, world_size=1)
    x, gw, ew, sc = draw_mx(cfg)
    x = block_factors(x)
    moe.set_weight_mx_scales(sc)
    out = torch.empty(256, 256, dtype=torch.bfloat16, device="cuda")
    st = torch.cuda.Stream()
    got = {}
    for mode in (None, "mxfp8", None):
        moe.set_activation_quant(mode)
        assert moe.get_activation_quant() == mode
        runs = [forward_raw(moe, cfg, x, gw, ew, out=out, stream=st).clone()
                for _ in range(4)]
        assert all(torch.equal(o, runs[0]) for o in runs)
        assert torch.equal(got.setdefault(mode, runs[0]), runs[0])
    assert not torch.equal(got["mxfp8"], got[None])
    _assert_mx_values(got["mxfp8"], reference(cfg, x, gw, ew, sc)["moe_out"])
    one = moe.moe_forward(x, gw, ew, activation_quant="mxfp8")
    assert lib().fm_get_activation_quant() == 3
    assert torch.equal(one.reshape(out.shape), got["mxfp8"])
    moe.finalize()
    moe.initialize(path, rank=0, world_size=1)
    assert lib().fm_get_activation_quant() == 0


@pytest.mark.parametrize("dtype", [4, 2])
def test_refusals(fresh_moe, dtype):
    cfg, path = make_cfg(**dict(BASE, torch_dtype=dtype))
    fresh_moe.initialize(path, rank=0, world_size=1)
    assert lib().fm_set_activation_quant(3) == FM_ERR_UNSUPPORTED
    assert b"torch_dtype" in lib().fm_last_error()
    assert b"mxfp8" in lib().fm_last_error()
    assert lib().fm_get_activation_quant() == 0
    with pytest.raises(ValueError, match="torch_dtype"):
        fresh_moe.set_activation_quant("mxfp8")
    assert lib().fm_get_activation_quant() == 0  # a refused call changes nothing
