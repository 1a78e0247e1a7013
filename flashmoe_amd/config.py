"""flashmoe_config.json contract (reference: csrc/flashmoe_config.json +
csrc/flashmoe_config.schema.json; loaded/validated at initialize time, the
MI355X analog of the reference's JSON -> CMake -D macro pipeline,
setup.py:223-292 / CMakeLists.txt:112-237)."""
from __future__ import annotations

import json
import os

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_CONFIG_PATH = os.path.join(REPO_ROOT, "csrc", "flashmoe_config.json")

REQUIRED_KEYS = [
    # csrc/flashmoe_config.schema.json "required"
    "capacity_factor", "drop_tokens", "expert_top_k", "is_training",
    "hidden_act", "hidden_size", "intermediate_size", "mini_batch",
    "moe_frequency", "num_experts", "num_layers", "sequence_len",
    "torch_dtype", "vocab_size",
]

# torch_dtype enum (schema): 0 float, 1 tf32 (== fp32 on CDNA4: no xf32),
# 2 bf16, 3 fp16, 4 fp8e4m3 expert weights with bf16 activations (the
# config-5 "fp8 weights / bf16 accumulate" regime), 5 MX fp8: fp8e4m3
# weights AND runtime-quantized fp8 activations (per-64-element E8M0
# block scales) on the CDNA4 scaled MFMA - the 2x-rate path (extension
# codes; the reference schema stops at 3). torch_dtype_of() is the
# ACTIVATION dtype at the API boundary; weight_dtype_of() the
# expert-weight storage dtype.
def torch_dtype_of(code: int):
    import torch

    return {0: torch.float32, 1: torch.float32, 2: torch.bfloat16,
            3: torch.float16, 4: torch.bfloat16, 5: torch.bfloat16}[code]


def weight_dtype_of(code: int):
    import torch

    if code in (4, 5):
        return torch.float8_e4m3fn
    return torch_dtype_of(code)


def element_size_of(code: int) -> int:
    # activation element size (workspace sizing); dtype-4 weights are 1B
    return {0: 4, 1: 4, 2: 2, 3: 2, 4: 2, 5: 2}[code]


# hidden_act enum (schema): 0 relu, 1 exact-erf gelu, 2 SwiGLU, 3 GeGLU.
# 2/3 are GATED experts: h = act(x.Wglu^T) * (x.Wup^T), and the expert
# weights carry a third [P, H] slab (slot 2 = Wglu): [nLx, 3, P, H].
def is_gated(hidden_act: int) -> bool:
    return hidden_act in (2, 3)


def expert_mats(hidden_act: int) -> int:
    """[P, H] slabs per expert in the expert-weights tensor (dim 1)."""
    return 3 if is_gated(hidden_act) else 2


# num_shared_experts (optional key, default 0): FFNs applied to EVERY token,
# unrouted and unscaled, and added to the routed result (DeepSeek-MoE /
# Qwen-MoE shared experts). Their slabs trail the routed ones:
# expert weights are [nLx + nSh, mats, P, H].
MAX_SHARED_EXPERTS = 4
MAX_COMBINE_SLOTS = 16  # the combine slot index j has four bits


def num_shared(cfg: dict) -> int:
    """Shared experts of a config (0 when the key is absent)."""
    return int(cfg.get("num_shared_experts", 0))


# Router keys (all optional; absent = the reference's router: softmax over
# all experts, plain top-k, weights p_j / sum_selected p). See
# fm_router_config in include/flashmoe_abi.h and DESIGN.md par.5j.
ROUTER_DEFAULTS = {
    "scoring_func": 0,           # 0 softmax, 1 sigmoid
    "norm_topk_prob": 1,         # 0: weights are the raw scores
    "n_group": 1,                # group-limited top-k (1 = no limit)
    "topk_group": 1,
    "group_score": 0,            # 0 max, 1 sum of the two largest
    "routed_scaling_factor": 1.0,
}
MAX_ROUTER_GROUPS = 16
MAX_VARIANT_EXPERTS = 256  # sigmoid / bias / groups: the route kernel's LDS


def router_of(cfg: dict) -> dict:
    """The router keys of a config with the defaults filled in."""
    return {k: cfg.get(k, d) for k, d in ROUTER_DEFAULTS.items()}


def router_is_default(cfg: dict) -> bool:
    return router_of(cfg) == ROUTER_DEFAULTS


def _validate_router(cfg: dict) -> None:
    """The fm_set_router refusals that the config alone decides (a score
    bias is attached later, moe.set_score_bias)."""
    import math

    r = router_of(cfg)
    E, k = cfg["num_experts"], cfg["expert_top_k"]
    for key in ("scoring_func", "norm_topk_prob", "group_score"):
        v = r[key]
        if isinstance(v, bool) or not isinstance(v, int) or v not in (0, 1):
            raise ValueError(f"{key} must be 0 or 1; got {v!r}")
    for key in ("n_group", "topk_group"):
        v = r[key]
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{key} must be an integer; got {v!r}")
    G, TG = r["n_group"], r["topk_group"]
    if not 1 <= G <= MAX_ROUTER_GROUPS:
        raise ValueError(f"n_group must be in [1, {MAX_ROUTER_GROUPS}]; got {G}")
    if E % G:
        raise ValueError(f"num_experts={E} is not divisible by n_group={G}")
    if not 1 <= TG <= G:
        raise ValueError(f"topk_group must be in [1, n_group={G}]; got {TG}")
    if k > TG * (E // G):
        raise ValueError(
            f"expert_top_k={k} exceeds the topk_group * num_experts / n_group "
            f"= {TG * (E // G)} experts of the kept groups")
    if r["group_score"] == 1 and E // G < 2:
        raise ValueError(
            f"group_score=1 (sum of top 2) needs at least 2 experts per "
            f"group; n_group={G} leaves {E // G}")
    f = r["routed_scaling_factor"]
    if isinstance(f, bool) or not isinstance(f, (int, float)) or \
            not math.isfinite(f) or f <= 0:
        raise ValueError(
            f"routed_scaling_factor must be a finite number > 0; got {f!r}")
    if k == 1 and r["norm_topk_prob"] == 0:
        raise ValueError(
            "norm_topk_prob=0 is not supported with expert_top_k=1: the "
            "top-1 direct store is unscaled")
    if k == 1 and float(f) != 1.0:
        raise ValueError(
            "routed_scaling_factor != 1 is not supported with expert_top_k=1: "
            "the top-1 direct store is unscaled")
    if cfg["is_training"] and not router_is_default(cfg):
        key = next(k_ for k_, d in ROUTER_DEFAULTS.items() if r[k_] != d)
        raise ValueError(
            f"a non-default {key} is not supported with is_training=1: the "
            "aux-loss accumulators are softmax-specific")
    if E > MAX_VARIANT_EXPERTS and (r["scoring_func"] == 1 or G > 1):
        key = "scoring_func=1" if r["scoring_func"] == 1 else f"n_group={G}"
        raise ValueError(
            f"{key} is not supported with num_experts > {MAX_VARIANT_EXPERTS} "
            "(the route kernel's LDS budget); norm_topk_prob and "
            "routed_scaling_factor work at every num_experts")


def num_tokens(cfg: dict) -> int:
    """S, the token count of one forward: sequence_len * mini_batch."""
    return cfg["sequence_len"] * cfg["mini_batch"]


def _validate_tokens(cfg: dict) -> None:
    """S = sequence_len * mini_batch is in 1..127 (decode-sized) or a
    positive multiple of 128, and the decode refusals that the config alone
    decides (world_size > 1 is refused at initialize)."""
    for key in ("sequence_len", "mini_batch"):
        v = cfg[key]
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{key} must be an integer; got {v!r}")
    S = num_tokens(cfg)
    if S < 1 or (S >= 128 and S % 128):
        raise ValueError(
            f"sequence_len * mini_batch = {S} must be in [1, 127] or a "
            "positive multiple of 128")
    if S < 128:
        if cfg["torch_dtype"] == 5:
            raise ValueError(
                f"torch_dtype=5 (MX fp8) is not supported with sequence_len * "
                f"mini_batch = {S} < 128 (decode-sized forwards)")
        if cfg["is_training"]:
            raise ValueError(
                f"is_training=1 is not supported with sequence_len * "
                f"mini_batch = {S} < 128 (decode-sized forwards)")


def load_config(path: str | None = None) -> dict:
    path = path or DEFAULT_CONFIG_PATH
    with open(path) as f:
        cfg = json.load(f)
    missing = [k for k in REQUIRED_KEYS if k not in cfg]
    if missing:
        raise ValueError(f"config {path} missing required keys: {missing}")
    _validate_tokens(cfg)
    if cfg["hidden_size"] % 64 or cfg["intermediate_size"] % 64:
        raise ValueError("hidden_size/intermediate_size must be multiples of 64 (schema)")
    if cfg["hidden_act"] not in (0, 1, 2, 3):
        raise ValueError(
            f"hidden_act must be 0 (relu), 1 (gelu), 2 (swiglu) or 3 (geglu); "
            f"got {cfg['hidden_act']}")
    nsh = cfg.get("num_shared_experts", 0)
    if isinstance(nsh, bool) or not isinstance(nsh, int) or \
            not 0 <= nsh <= MAX_SHARED_EXPERTS:
        raise ValueError(
            f"num_shared_experts must be an integer in "
            f"[0, {MAX_SHARED_EXPERTS}]; got {nsh!r}")
    if cfg["expert_top_k"] + nsh > MAX_COMBINE_SLOTS:
        raise ValueError(
            f"expert_top_k + num_shared_experts must be <= "
            f"{MAX_COMBINE_SLOTS}; got {cfg['expert_top_k']} + {nsh}")
    if nsh > 0 and cfg["torch_dtype"] == 5:
        raise ValueError(
            f"num_shared_experts={nsh} is not supported with torch_dtype=5 "
            "(MX fp8): shared experts occur in gated models, and gated + MX "
            "is itself unsupported")
    if is_gated(cfg["hidden_act"]) and cfg["torch_dtype"] == 5:
        raise ValueError(
            f"hidden_act={cfg['hidden_act']} (gated) is not supported with "
            "torch_dtype=5 (MX fp8): the MX up epilogue cannot yet halve its "
            "output width")
    _validate_router(cfg)
    return cfg
