"""Single-GPU shape benchmark for any BASELINE-like MoE shape.

Usage: python tools/shape_bench.py [--hidden-act A] [--shared N | --compose N]
                                   [--router qwen|v2|v3|sigmoid]
                                   [--weight-scales]
                                   [S H P E topk [steps [dtype]]]
Defaults to the BASELINE config-3 shape. Prints one JSON line with
per-phase HIP-event timing (fm_moe_forward_phased). --hidden-act 2/3
times a gated (SwiGLU/GeGLU) expert with [E, 3, P, H] weights.
--shared N times a config with num_shared_experts = N ([E + N, ...]
weights, the shared experts folded into the two expert GEMM launches).
--compose N times the hand composition of the same result on a config
WITHOUT the key: moe_forward on the routed slabs, fm_expert_ffn over all S
rows per shared slab, and a torch add (us_per_fwd only covers the whole
composition; the phase times are those of the routed forward alone).
--router times a router variant: qwen = softmax without
renormalisation; v2 = DeepSeek-V2 (groups 8/3 by max, no renormalisation,
factor 16); v3 = DeepSeek-V3 (sigmoid + bias, groups 8/4 by top-2 sum,
renormalised, factor 2.5); sigmoid = sigmoid + bias, renormalised, no groups.
Its gate weights are scaled by 1/sqrt(H), the bias is 0.1 * randn(E).
S may be a comma list (1,8,32,64): one JSON line per S, the weights drawn
once. --mini-batch writes the config as sequence_len 1, mini_batch S (the
decode form; S = sequence_len * mini_batch either way). Every line carries
weight_bytes, the bytes of all weight slabs of the routed experts with rows
(from the fm_read_routing counts) and of the shared experts, both phases, each
counted once, and floor_us = weight_bytes /
6.3 TB/s, a bytes bound. --decode-ab R (S < 128) times R
runs of `steps` forwards under FM_DECODE_FFN=1 and R under =0, alternated,
and reports every run. --weight-scales (dtype 4 and 5 only, DESIGN.md
par.5l) attaches a random per-output-channel weight-scale tensor,
exp2(U(-2, 1)) per channel.
"""
import ctypes
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import flashmoe_amd._ext as _ext
from flashmoe_amd import moe

argv = sys.argv[1:]
hidden_act = 0
if "--hidden-act" in argv:
    i = argv.index("--hidden-act")
    hidden_act = int(argv[i + 1])
    del argv[i:i + 2]
n_shared = n_compose = 0
for flag in ("--shared", "--compose"):
    if flag in argv:
        i = argv.index(flag)
        if flag == "--shared":
            n_shared = int(argv[i + 1])
        else:
            n_compose = int(argv[i + 1])
        del argv[i:i + 2]
ROUTERS = {
    "qwen": dict(norm_topk_prob=0),
    "v2": dict(n_group=8, topk_group=3, group_score=0, norm_topk_prob=0,
               routed_scaling_factor=16.0),
    "v3": dict(scoring_func=1, n_group=8, topk_group=4, group_score=1,
               norm_topk_prob=1, routed_scaling_factor=2.5),
    "sigmoid": dict(scoring_func=1, norm_topk_prob=1),
}
router = None
if "--router" in argv:
    i = argv.index("--router")
    router = argv[i + 1]
    del argv[i:i + 2]
mini_batch_form = "--mini-batch" in argv
if mini_batch_form:
    argv.remove("--mini-batch")
weight_scales = "--weight-scales" in argv
if weight_scales:
    argv.remove("--weight-scales")
ab_runs = 0
if "--decode-ab" in argv:
    i = argv.index("--decode-ab")
    ab_runs = int(argv[i + 1])
    del argv[i:i + 2]
s_list = None
if argv and "," in argv[0]:
    s_list = [int(v) for v in argv[0].split(",")]
    argv[0] = str(s_list[0])
args = [int(a) for a in argv]
S, H, P, E, topk = (args + [4096, 2048, 8192, 64, 2][len(args):])[:5]
s_list = s_list or [S]
steps = args[5] if len(args) > 5 else 30
dtype_code = args[6] if len(args) > 6 else 2

from flashmoe_amd.config import expert_mats, torch_dtype_of, weight_dtype_of

if weight_scales and dtype_code not in (4, 5):
    sys.exit("--weight-scales needs fp8 expert weights: dtype 4 or 5")

adt, wdt = torch_dtype_of(dtype_code), weight_dtype_of(dtype_code)
torch.manual_seed(47)
x_first = torch.randn(1, s_list[0], H, dtype=adt, device="cuda")
gw = torch.randn(H, E, dtype=adt, device="cuda")
if router:
    gw = (gw.float() / H ** 0.5).to(adt)
score_bias = None
if router in ("v3", "sigmoid"):
    score_bias = 0.1 * torch.randn(E, dtype=torch.float32, device="cuda")
ew_all = torch.randn(E + n_shared + n_compose, expert_mats(hidden_act), P, H,
                     dtype=torch.float32, device="cuda").to(wdt)
ew = ew_all[:E + n_shared]  # what moe_forward sees (a leading slice)
w_scales = None
if weight_scales:
    # a generator of its own: the inputs drawn later stay those of a run
    # without the flag
    w_scales = torch.exp2(3.0 * torch.rand(
        E + n_shared, P + H + (P if expert_mats(hidden_act) == 3 else 0),
        dtype=torch.float32, device="cuda",
        generator=torch.Generator(device="cuda").manual_seed(48)) - 2.0)
lib = _ext.load()
HBM_ACHIEVABLE = 6.3e12  # bytes/s


def measure(S):
    cfg = {"capacity_factor": 1, "drop_tokens": 1, "expert_top_k": topk,
           "global_batch": 256, "is_training": 0, "hidden_act": hidden_act,
           "hidden_size": H, "intermediate_size": P,
           "mini_batch": S if mini_batch_form else 1,
           "moe_frequency": 1, "num_experts": E, "num_layers": 1,
           "sequence_len": 1 if mini_batch_form else S,
           "torch_dtype": dtype_code, "vocab_size": 32000}
    if n_shared:
        cfg["num_shared_experts"] = n_shared
    if router:
        cfg.update(ROUTERS[router])
    f = tempfile.NamedTemporaryFile("w", suffix=".json", delete=False)
    json.dump(cfg, f)
    f.close()
    moe.initialize(f.name, rank=0, world_size=1)
    os.unlink(f.name)
    if score_bias is not None:
        moe.set_score_bias(score_bias)
    if w_scales is not None:
        moe.set_weight_scales(w_scales)
    x = x_first if S == s_list[0] else \
        torch.randn(1, S, H, dtype=adt, device="cuda")
    x = x.view(cfg["mini_batch"], cfg["sequence_len"], H)
    sh_out = torch.empty(S, H, dtype=adt, device="cuda")

    def forward():
        out = moe.moe_forward(x, gw, ew)
        if n_compose:
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            for s_ in range(n_compose):
                _ext.check(lib.fm_expert_ffn(
                    st, ctypes.c_void_p(x.data_ptr()),
                    ctypes.c_void_p(ew_all.data_ptr()), None, None,
                    ctypes.c_void_p(sh_out.data_ptr()), S, E + s_),
                    "fm_expert_ffn")
                out = out + sh_out.view_as(out)
        return out

    def timed():
        for _ in range(max(3, steps // 3)):
            forward()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            forward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    ab = None
    if ab_runs and S < 128:
        saved = os.environ.get("FM_DECODE_FFN")
        ab = {"ffn1_us": [], "ffn0_us": []}
        for _ in range(ab_runs):
            for arm in ("1", "0"):
                os.environ["FM_DECODE_FFN"] = arm
                ab[f"ffn{arm}_us"].append(round(timed() * 1e6, 1))
        if saved is None:
            os.environ.pop("FM_DECODE_FFN", None)
        else:
            os.environ["FM_DECODE_FFN"] = saved
    dt = timed()

    ms = (ctypes.c_float * 4)()
    acc = [0.0] * 4
    out = torch.empty_like(x)
    go = moe.gate_output()
    for _ in range(5):
        _ext.check(lib.fm_moe_forward_phased(
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
            ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(gw.data_ptr()),
            ctypes.c_void_p(ew.data_ptr()), None, None,
            ctypes.c_void_p(go.data_ptr()), ctypes.c_void_p(out.data_ptr()),
            S, ms), "phased")
        for i in range(4):
            acc[i] += ms[i] / 5
    # the weight bytes one forward has to stream at least once: every slab
    # of every routed expert with rows and of every shared expert, up and
    # down phase together (a bytes floor: the row slices of a shared expert
    # and the row passes of k_decode_ffn beyond 32 rows re-read slabs, which
    # the floor does not count)
    base = -(-S // E)
    EC = base * topk
    import numpy as np

    counts = np.zeros(E, dtype=np.uint32)
    tok = np.zeros(E * EC, dtype=np.uint32)
    ps = np.zeros(E * EC, dtype=np.float32)
    _ext.check(lib.fm_read_routing(
        None, ctypes.c_void_p(counts.ctypes.data),
        ctypes.c_void_p(tok.ctypes.data), ctypes.c_void_p(ps.ctypes.data)),
        "fm_read_routing")
    hit = int((counts > 0).sum())
    weight_bytes = ((hit + n_shared) * expert_mats(hidden_act) * P * H *
                    ew.element_size())
    flops = 4.0 * S * topk * H * P  # upper bound (pre-capacity-drop)
    gemm_ms = acc[1] + acc[2]
    res = {
        "workload": (f"1xMI355X S={S} H={H} P={P} E={E} top-{topk} "
                     f"dtype{dtype_code} act{hidden_act} CF=1 drop"
                     + (f" shared={n_shared}" if n_shared else "")
                     + (f" compose={n_compose}" if n_compose else "")
                     + (f" router={router}" if router else "")
                     + (" weight-scales" if weight_scales else "")),
        "us_per_fwd": round(dt * 1e6, 1),
        "tokens_per_s": round(S / dt),
        "gemm_tflops_upper": round(flops / gemm_ms / 1e9, 1) if gemm_ms else None,
        "phase_ms": {"gate": round(acc[0], 4), "up": round(acc[1], 4),
                     "down": round(acc[2], 4), "other": round(acc[3], 4)},
        "experts_hit": hit,
        "weight_bytes": weight_bytes,
        "floor_us": round(weight_bytes / HBM_ACHIEVABLE * 1e6, 1),
    }
    if ab:
        res["decode_ab"] = ab
    print(json.dumps(res), flush=True)
    moe.finalize()


for S_ in s_list:
    measure(S_)
