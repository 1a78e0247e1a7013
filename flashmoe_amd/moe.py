"""Host-side mirror of the reference's pybind11 module `flashmoe._C`
(csrc/python_bindings.cu:194-217): initialize / moe_forward / finalize /
get_compiled_config / get_num_local_experts — same names, argument meaning
and error behaviour, implemented over the C-ABI (include/flashmoe_abi.h).
"""
from __future__ import annotations

import ctypes
import os

from . import _ext
from .config import (MAX_VARIANT_EXPERTS, element_size_of, expert_mats,
                     load_config, num_shared, num_tokens, router_is_default,
                     router_of,
                     torch_dtype_of, weight_dtype_of)

_state = {
    "initialized": False,
    "cfg": None,
    "rank": 0,
    "world": 1,
    "gate_out": None,  # persistent [S, PX] buffer (internal, like the
    # reference's flat-buffer gate output, python_bindings.cu:70-74)
    "score_bias": None,  # the fp32 [E] tensor fm_set_router borrows
    "weight_scales": None,  # the fp32 tensor fm_set_weight_scales borrows
}


def _check_cuda():
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError(
            "FlashMoE-AMD requires a ROCm GPU (gfx950); torch.cuda.is_available() is False"
        )


def initialize(config_path: str | None = None, rank: int | None = None,
               world_size: int | None = None):
    """Mirror of _C.initialize (python_bindings.cu:157-159).

    rank/world default from torch.distributed env vars (RANK/WORLD_SIZE)
    when present, else single process.
    """
    import torch

    if _state["initialized"]:
        raise RuntimeError("initialize() already called")
    _check_cuda()
    lib = _ext.load()  # fails loudly if the HIP extension is missing
    cfg = load_config(config_path)
    if rank is None:
        rank = int(os.environ.get("RANK", "0"))
    if world_size is None:
        world_size = int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(rank % torch.cuda.device_count())
    c = _ext.FMConfig(
        num_experts=cfg["num_experts"],
        expert_top_k=cfg["expert_top_k"],
        capacity_factor=cfg["capacity_factor"],
        drop_tokens=cfg["drop_tokens"],
        hidden_act=cfg["hidden_act"],
        hidden_size=cfg["hidden_size"],
        intermediate_size=cfg["intermediate_size"],
        sequence_len=cfg["sequence_len"],
        mini_batch=cfg["mini_batch"],
        dtype=cfg["torch_dtype"],
        is_training=cfg["is_training"],
        num_shared_experts=num_shared(cfg),
    )
    _ext.check(lib.fm_initialize(ctypes.byref(c), rank, world_size), "fm_initialize")
    _state.update(initialized=True, cfg=cfg, rank=rank, world=world_size,
                  score_bias=None, weight_scales=None)
    if not router_is_default(cfg):
        try:
            _apply_router()
        except Exception:
            lib.fm_finalize()
            _state.update(initialized=False, cfg=None)
            raise
    # persistent gate_out buffer
    S = num_tokens(cfg)
    PX = (cfg["num_experts"] + 63) // 64 * 64
    _state["gate_out"] = torch.empty(
        S, PX, dtype=torch_dtype_of(cfg["torch_dtype"]), device="cuda"
    )


def finalize():
    """Mirror of _C.finalize (python_bindings.cu:163-168)."""
    if not _state["initialized"]:
        raise RuntimeError("finalize() before initialize()")
    _ext.check(_ext.load().fm_finalize(), "fm_finalize")
    _state.update(initialized=False, cfg=None, gate_out=None, score_bias=None,
                  weight_scales=None)
    _state.pop("p2p", None)        # heap freed by fm_finalize
    _state.pop("ep_buffers", None)
    # a P2P setup failure is scoped to one initialize/finalize cycle
    _state.pop("p2p_failed", None)
    _state.pop("p2p_validated", None)


def _apply_router():
    """fm_set_router from the config's router keys and the current bias."""
    r = router_of(_state["cfg"])
    bias = _state["score_bias"]
    c = _ext.FMRouterConfig(
        scoring_func=r["scoring_func"], norm_topk_prob=r["norm_topk_prob"],
        n_group=r["n_group"], topk_group=r["topk_group"],
        group_score=r["group_score"],
        routed_scaling_factor=float(r["routed_scaling_factor"]),
        score_bias=bias.data_ptr() if bias is not None else None)
    _ext.check(_ext.load().fm_set_router(ctypes.byref(c)), "fm_set_router")


def set_score_bias(bias):
    """Attach (or, with None, detach) the selection bias of the router:
    a contiguous fp32 [E] CUDA tensor added to the scores for SELECTION
    only, never to the weights (DeepSeek-V3's e_score_correction_bias).
    The tensor is borrowed by the library and kept alive here; its contents
    may be rewritten in place between forwards."""
    import torch

    if not _state["initialized"]:
        raise RuntimeError("Must call initialize() first")
    if bias is not None:
        E = _state["cfg"]["num_experts"]
        if not isinstance(bias, torch.Tensor) or not bias.is_cuda:
            raise ValueError("score bias must be a CUDA tensor")
        if bias.dtype != torch.float32 or tuple(bias.shape) != (E,) or \
                not bias.is_contiguous():
            raise ValueError(
                f"score bias must be a contiguous float32 [E={E}] tensor; got "
                f"{bias.dtype} {tuple(bias.shape)}")
        if E > MAX_VARIANT_EXPERTS:
            raise ValueError(
                f"a score bias is not supported with num_experts > "
                f"{MAX_VARIANT_EXPERTS} (the route kernel's LDS budget)")
    prev = _state["score_bias"]
    _state["score_bias"] = bias
    try:
        _apply_router()
    except Exception:
        _state["score_bias"] = prev
        raise


def get_router() -> dict:
    """The active router (fm_get_router): the config keys plus
    "score_bias", the attached tensor or None."""
    if not _state["initialized"]:
        raise RuntimeError("Must call initialize() first")
    c = _ext.FMRouterConfig()
    _ext.check(_ext.load().fm_get_router(ctypes.byref(c)), "fm_get_router")
    bias = _state["score_bias"]
    assert (c.score_bias or 0) == (bias.data_ptr() if bias is not None else 0)
    return {"scoring_func": c.scoring_func, "norm_topk_prob": c.norm_topk_prob,
            "n_group": c.n_group, "topk_group": c.topk_group,
            "group_score": c.group_score,
            "routed_scaling_factor": float(c.routed_scaling_factor),
            "score_bias": bias}


def _weight_scale_shape():
    """(records, SC) of the weight-scale tensor for the initialized config:
    one record [s_up (P) | s_dn (H) | s_glu (P, gated only)] per local routed
    expert, then one per shared expert."""
    cfg = _state["cfg"]
    P, H = cfg["intermediate_size"], cfg["hidden_size"]
    n = _ext.load().fm_get_num_local_experts() + num_shared(cfg)
    return n, P + H + (P if expert_mats(cfg["hidden_act"]) == 3 else 0)


def set_weight_scales(scales):
    """Attach (or, with None, detach) per-output-channel fp32 scales of the
    fp8 expert weights (torch_dtype 4 and 5): W_eff[r, :] = W_fp8[r, :] * s[r],
    applied to the fp32 accumulators ahead of bias and activation (DESIGN.md
    par.5l). `scales` is a contiguous float32 CUDA tensor [nLx + nSh, SC] as
    built by pack_weight_scales. The tensor is borrowed by the library and
    kept alive here; its contents may be rewritten in place between
    forwards."""
    import torch

    if not _state["initialized"]:
        raise RuntimeError("Must call initialize() first")
    lib = _ext.load()
    if scales is None:
        _ext.check(lib.fm_set_weight_scales(None, 0), "fm_set_weight_scales")
        _state["weight_scales"] = None
        return
    dt = _state["cfg"]["torch_dtype"]
    if dt not in (4, 5):
        raise ValueError(
            f"weight scales need fp8 expert weights (torch_dtype 4 or 5); the "
            f"initialized config has torch_dtype {dt}")
    want = _weight_scale_shape()
    if not isinstance(scales, torch.Tensor) or not scales.is_cuda:
        raise ValueError(
            f"weight scales must be a CUDA float32 tensor of shape "
            f"[nLx + nSh, SC] = {list(want)}")
    if scales.dtype != torch.float32 or tuple(scales.shape) != want or \
            not scales.is_contiguous():
        raise ValueError(
            f"weight scales must be a contiguous float32 tensor of shape "
            f"[nLx + nSh, SC] = {list(want)}; got {scales.dtype} "
            f"{list(scales.shape)}")
    _ext.check(lib.fm_set_weight_scales(ctypes.c_void_p(scales.data_ptr()), 1),
               "fm_set_weight_scales")
    _state["weight_scales"] = scales


def get_weight_scales():
    """The attached weight-scale tensor, or None, as the library reports it
    (fm_get_weight_scales). Scales attached through the raw C-ABI are not a
    tensor this module holds: RuntimeError."""
    if not _state["initialized"]:
        raise RuntimeError("Must call initialize() first")
    ptr, gran = ctypes.c_void_p(), ctypes.c_int32()
    _ext.check(_ext.load().fm_get_weight_scales(ctypes.byref(ptr),
                                                ctypes.byref(gran)),
               "fm_get_weight_scales")
    if gran.value == 0:
        return None
    t = _state["weight_scales"]
    if t is None or t.data_ptr() != (ptr.value or 0):
        raise RuntimeError(
            f"weight scales at {ptr.value or 0:#x} (granularity {gran.value}) "
            f"were attached through fm_set_weight_scales directly, not through "
            f"set_weight_scales: there is no tensor to return")
    return t


def pack_weight_scales(up, down, glu=None):
    """Build the [nE, SC] weight-scale tensor from per-matrix scales: `up`
    [nE, P] (rows of Wup), `down` [nE, H] (rows of the down buffer used as
    [H, P]) and, for gated experts, `glu` [nE, P]. nE counts the shared
    experts, which come last. Every size-1 dimension broadcasts, and a 0-dim
    or 1-D [nE] tensor is a per-tensor scale: [nE], [nE, 1], [1] and 0-dim all
    spread over the channels (and the last two over the experts). nE, P and H
    come from the dimensions larger than 1, else from the initialized config.
    Returns a contiguous float32 tensor on the device of the first argument
    that has channels, with records [s_up | s_dn | s_glu]."""
    import torch

    named = [("up", up), ("down", down)] + ([("glu", glu)] if glu is not None
                                            else [])
    parts = []
    for name, t in named:
        t = torch.as_tensor(t, dtype=torch.float32)
        if t.dim() > 2:
            raise ValueError(f"{name} scales must have at most 2 dimensions; "
                             f"got {list(t.shape)}")
        # 0-dim -> [1, 1]; [n] -> [n, 1]: one value per expert
        parts.append(t.reshape(t.size(0) if t.dim() else 1, -1))

    def agreed(what, sizes, fallback):
        """The one size > 1 among `sizes`; `fallback` when all broadcast."""
        big = sorted({n for n in sizes if n != 1})
        if len(big) > 1:
            raise ValueError(f"pack_weight_scales: the arguments disagree on "
                             f"{what}: {big}")
        if big:
            return big[0]
        if fallback is None:
            raise ValueError(
                f"pack_weight_scales cannot infer {what} from broadcast "
                f"(size-1) arguments alone: pass it in a tensor's shape, or "
                f"call after initialize()")
        return fallback

    cfg = _state["cfg"]
    nE = agreed("the expert count nE", [t.size(0) for t in parts],
                _weight_scale_shape()[0] if cfg else 1)
    P = agreed("P", [t.size(1) for t in parts[0::2]],
               cfg["intermediate_size"] if cfg else None)
    H = agreed("H", [parts[1].size(1)], cfg["hidden_size"] if cfg else None)
    dev = next((t.device for t in parts if t.size(1) != 1), parts[0].device)
    cols = [t.to(dev).expand(nE, w) for t, w in zip(parts, (P, H, P))]
    return torch.cat(cols, dim=1).contiguous()


def get_compiled_config() -> dict:
    """Mirror of _C.get_compiled_config (python_bindings.cu:170-183 /
    ops.py:63-71): dict with S, H, E, P, PX, element_size_bytes."""
    if not _state["initialized"]:
        # the reference reads compile-time constants without initialize;
        # we read the default config file (same contract)
        cfg = load_config()
        S = num_tokens(cfg)
        return {
            "S": S,
            "H": cfg["hidden_size"],
            "E": cfg["num_experts"],
            "P": cfg["intermediate_size"],
            "PX": (cfg["num_experts"] + 63) // 64 * 64,
            "element_size_bytes": element_size_of(cfg["torch_dtype"]),
        }
    lib = _ext.load()
    vals = [ctypes.c_int64() for _ in range(6)]
    _ext.check(lib.fm_get_compiled_config(*[ctypes.byref(v) for v in vals]),
               "fm_get_compiled_config")
    S, H, E, P, PX, esz = [int(v.value) for v in vals]
    return {"S": S, "H": H, "E": E, "P": P, "PX": PX, "element_size_bytes": esz}


def get_num_local_experts() -> int:
    """Mirror of _C.get_num_local_experts (python_bindings.cu:185-189):
    the ROUTED local experts; shared experts are not counted."""
    if not _state["initialized"]:
        raise RuntimeError("Must call initialize() first")
    return _ext.load().fm_get_num_local_experts()


def get_num_shared_experts() -> int:
    """num_shared_experts of the initialized config: the expert-weights
    tensor carries this many slabs after the routed ones."""
    if not _state["initialized"]:
        raise RuntimeError("Must call initialize() first")
    return _ext.load().fm_get_num_shared_experts()


def _validate_forward_args(input, gate_weights, expert_weights):
    """Shape/device/contiguity validation mirroring the reference's
    TORCH_CHECKs (python_bindings.cu:22-70) against the frozen config."""
    import torch

    if not _state["initialized"]:
        raise RuntimeError("Must call initialize() before moe_forward")
    cc = get_compiled_config()
    S, H, E, P = cc["S"], cc["H"], cc["E"], cc["P"]
    nLx = get_num_local_experts()
    for name, t in (("Input", input), ("Gate weights", gate_weights),
                    ("Expert weights", expert_weights)):
        if not t.is_cuda:
            raise ValueError(f"{name} must be CUDA tensor")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if input.dim() != 3:
        raise ValueError("Input must be 3D [batch, seq, H]")
    if input.size(0) * input.size(1) != S:
        raise ValueError(
            f"Input batch*seq must equal compiled S={S}. Got batch={input.size(0)}, "
            f"seq={input.size(1)} (product={input.size(0) * input.size(1)})"
        )
    if input.size(2) != H:
        raise ValueError(f"Input hidden_size must equal compiled H={H}. Got {input.size(2)}")
    if tuple(gate_weights.shape) != (H, E):
        raise ValueError(
            f"Gate weights must be [H={H}, E={E}]. Got "
            f"[{gate_weights.size(0)}, {gate_weights.size(1)}]"
        )
    nSh = get_num_shared_experts()
    if expert_weights.size(0) != nLx + nSh:
        if nSh:
            raise ValueError(
                f"Expert count mismatch. Expected {nLx} local + {nSh} shared "
                f"experts ([{nLx + nSh}, ...], num_shared_experts={nSh}), "
                f"got {expert_weights.size(0)}")
        raise ValueError(
            f"Expert count mismatch. Expected {nLx} local experts, got {expert_weights.size(0)}"
        )
    act = _state["cfg"]["hidden_act"]
    nm = expert_mats(act)
    if expert_weights.size(1) != nm:
        if nm == 3:
            raise ValueError(
                f"Expert weights must have up, down and gating projections "
                f"[nLx, 3, P, H] for the gated hidden_act={act}. Got dim 1 = "
                f"{expert_weights.size(1)}")
        raise ValueError("Expert weights must have up and down projections [nLx, 2, P, H]")
    if expert_weights.size(2) != P or expert_weights.size(3) != H:
        raise ValueError(
            f"Expert weights must be [*, {nm}, P={P}, H={H}]. Got "
            f"[*, {nm}, {expert_weights.size(2)}, {expert_weights.size(3)}]"
        )
    expect_dtype = torch_dtype_of(_state["cfg"]["torch_dtype"])
    expect_wdtype = weight_dtype_of(_state["cfg"]["torch_dtype"])
    for name, t, want in (("Input", input, expect_dtype),
                          ("Gate weights", gate_weights, expect_dtype),
                          ("Expert weights", expert_weights, expect_wdtype)):
        if t.dtype != want:
            raise ValueError(f"{name} dtype {t.dtype} != compiled {want}")
    return S, H, E, P, nLx


def moe_forward(input, gate_weights, expert_weights, weight_scales=None):
    """Mirror of _C.moe_forward (python_bindings.cu:17-151): one DMoE
    forward on this rank's tokens. Single-rank path; world>1 uses the EP
    pipeline in ep.py (same result per rank). With
    num_shared_experts = nSh > 0 expert_weights is [nLx + nSh, mats, P, H]
    (shared slabs last) and every token also receives the unscaled sum of
    the shared FFNs. weight_scales (torch_dtype 4 / 5): a
    tensor as for set_weight_scales; one that is not the attached tensor is
    attached first, None leaves the attachment as it is."""
    import torch

    S, H, E, P, nLx = _validate_forward_args(input, gate_weights, expert_weights)
    if weight_scales is not None and weight_scales is not _state["weight_scales"]:
        set_weight_scales(weight_scales)
    if _state["world"] != 1:
        from . import ep

        return ep.moe_forward_ep(input, gate_weights, expert_weights)
    lib = _ext.load()
    out = torch.empty_like(input)
    gate_out = _state["gate_out"]
    stream = torch.cuda.current_stream().cuda_stream
    _ext.check(
        lib.fm_moe_forward(
            ctypes.c_void_p(stream),
            ctypes.c_void_p(input.data_ptr()),
            ctypes.c_void_p(gate_weights.data_ptr()),
            ctypes.c_void_p(expert_weights.data_ptr()),
            None,
            None,
            ctypes.c_void_p(gate_out.data_ptr()),
            ctypes.c_void_p(out.data_ptr()),
            S,
        ),
        "fm_moe_forward",
    )
    return out


def gate_output():
    """The [S, PX] scores of the last forward: softmax probabilities, or
    sigmoid scores under scoring_func 1 (the reference exposes these as the
    first slab of its output buffer, moe.cuh:128-131)."""
    return _state["gate_out"]
