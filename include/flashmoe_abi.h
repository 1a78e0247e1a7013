/* C-ABI boundary of the MI355X-native FlashDMoE hot path.
 *
 * Each entry point cites the reference interface it replaces
 * (file:line into /root/reference). No torch types: plain pointers,
 * sizes and an opaque HIP stream. All device pointers are raw HIP
 * device memory on the current device; the caller owns input/output
 * buffers, the library owns its internal workspace.
 *
 * Threading model: one process per GPU, all calls from
 * one host thread per process, kernels enqueued on the caller's stream.
 *
 * The Python mirror (flashmoe_amd/moe.py, ctypes) reproduces the
 * reference's pybind11 surface `flashmoe._C`
 * (csrc/python_bindings.cu:194-217) on top of these functions; the
 * binding stub a maintainer would add upstream is in INTEGRATION.md.
 */
#ifndef FLASHMOE_ABI_H
#define FLASHMOE_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Error codes (negative) / 0 on success. fm_last_error() returns a
 * human-readable message for the most recent failure on this thread. */
#define FM_OK 0
#define FM_ERR_HIP (-1)          /* HIP runtime failure */
#define FM_ERR_STATE (-2)        /* initialize/finalize ordering */
#define FM_ERR_SHAPE (-3)        /* shape mismatch vs frozen config */
#define FM_ERR_UNSUPPORTED (-4)  /* dtype/feature not built */

/* Mirror of csrc/flashmoe_config.json (schema:
 * csrc/flashmoe_config.schema.json). dtype: 0 fp32, 1 tf32(=fp32 on
 * CDNA4 - no xf32), 2 bf16, 3 fp16, 4 fp8e4m3 expert weights with bf16
 * activations (W8A16), 5 MX-block-scaled fp8: fp8e4m3 weights AND
 * runtime-quantized fp8 activations (per-64-element E8M0 block scales)
 * on the CDNA4 scaled MFMA; weights are passed exactly as for dtype 4,
 * activation quantization is internal. dtype 5 requires H, P multiples
 * of 128. For dtype 4 and 5 the weight scale is 1.0 unless scales are
 * attached with fm_set_weight_scales (per output channel, below).
 *
 * hidden_act: 0 relu, 1 exact-erf gelu: z = act(x.Wup^T + b_up).Wdn^T + b_dn
 * with expert weights [nLx, 2, P, H]. 2 SwiGLU (silu(v) = v / (1 + exp(-v)))
 * and 3 GeGLU (exact-erf gelu) are GATED experts:
 *   h = act(x.Wglu^T) * (x.Wup^T), z = h.Wdn^T + b_dn
 * computed in fp32 from the fp32 accumulators and rounded once to Element.
 * Gated expert weights are [nLx, 3, P, H]: slot 0 = Wup [P,H], slot 1 =
 * the down buffer (flat, used as [H,P]) - both exactly as for the
 * two-slab layout - and slot 2 = the gating projection Wglu [P,H]; the
 * expert stride is 3*P*H. Unsupported with a gated hidden_act
 * (FM_ERR_UNSUPPORTED): b_up != NULL (every entry point), and dtype 5
 * (at fm_initialize). Gated forwards always run the multi-kernel path,
 * never the single-launch fused kernel.
 *
 * num_shared_experts (nSh, 0..4, expert_top_k + nSh <= 16): SHARED experts,
 * FFNs applied to every token, unrouted and unscaled, and added to the
 * routed result (DeepSeek-MoE / Qwen-MoE):
 *   moe_out[t] = Element( sum_{j<k, kept} Element(scale_j * FFN_{e_j}(x_t))
 *                       + sum_{s<nSh} Element(FFN_{nLx+s}(x_t)) )
 * summed in fp32 in that order, rounded once. The routed terms are exactly
 * those of nSh == 0; a token whose routed slots were all dropped still
 * receives its shared terms. Shared experts use the config's hidden_act, P
 * and dtype; their weight slabs TRAIL the routed ones in the same slot
 * layout, so expert_w is [nLx + nSh, mats, P, H] and b_up / b_dn, where
 * given, are [nLx + nSh, P] / [nLx + nSh, H] (indexed by weight-expert
 * id). A shared expert of width n*P is exactly the sum of n shared experts
 * of width P (column split of Wup/Wglu, row split of Wdn). They run as extra
 * z-slices of the two grouped expert GEMM launches of fm_moe_forward /
 * fm_moe_forward_phased (always the multi-kernel path). The staged entry
 * points (fm_gate_forward, fm_expert_ffn*, fm_combine*) ignore them;
 * fm_expert_ffn can address a shared slab with local_e = nLx + s.
 * FM_ERR_UNSUPPORTED at fm_initialize: nSh outside 0..4, expert_top_k +
 * nSh > 16, nSh > 0 with dtype 5, nSh > 0 with world_size > 1.
 *
 * DECODE-SIZED FORWARDS: S = sequence_len * mini_batch may be any integer in
 * 1..127 as well as a positive multiple of 128 (the rule is on the product:
 * sequence_len 1, mini_batch 8 is the natural decode config). One config is
 * one S. Below 128 the gate runs as one masked tile (rows >= S are neither
 * read nor written, so gate_out is exactly [S, PX] and moe_out exactly
 * [S, H]; the placement is deterministic, overflow included). For dtype
 * 2/3/4 there are weight-streaming expert FFN kernels that skip the weights
 * of experts without rows; they are the default at S <= 4 (dtype 2), S <= 8
 * (dtype 3) and S <= 16 (dtype 4), the grouped GEMMs above that
 * (FM_DECODE_FFN=0 forces the grouped GEMMs, =1 the streaming kernels;
 * re-read per call; fm_last_forward_decode_ffn() reports which ran). Supported: dtype 0-4, every
 * hidden_act, b_up (ungated) / b_dn, top-1..8, drop and no-drop,
 * num_shared_experts, every router variant; fm_moe_forward,
 * fm_moe_forward_phased, fm_gate_forward, fm_read_routing, fm_export_routing.
 * FM_ERR_UNSUPPORTED at fm_initialize with S < 128: dtype 5, is_training 1,
 * world_size > 1. S >= 128 that is no multiple of 128: FM_ERR_SHAPE. A
 * decode-sized forward never takes the single-launch kernels
 * (fm_last_forward_fused() reports 0).
 *
 * ABI NOTE: the struct GREW by this trailing field. A caller built against
 * the eleven-field layout must be rebuilt (or zero the new field). */
typedef struct fm_config {
  int32_t num_experts;
  int32_t expert_top_k;
  int32_t capacity_factor;
  int32_t drop_tokens;
  int32_t hidden_act; /* 0 relu, 1 gelu, 2 swiglu, 3 geglu (see above) */
  int32_t hidden_size;        /* H */
  int32_t intermediate_size;  /* P */
  int32_t sequence_len;  /* sequence_len * mini_batch (= S, the token
                          * count) must be in 1..127 (decode-sized, see
                          * above) or a positive multiple of 128: the gate
                          * tiles tokens in blocks of 128 and masks at most
                          * the one ragged tile of S < 128 */
  int32_t mini_batch;
  int32_t dtype;
  int32_t is_training;
  int32_t num_shared_experts; /* 0 = none (see above); last field */
} fm_config;

/* Replaces flashmoe::initialize (python_bindings.cu:157-159,
 * bootstrap.cuh:533-547): freezes the config, selects the device,
 * allocates the library workspace (tokenIds, eC, xM, O32) sized from the
 * config. rank/world describe the EP layout (nLx = num_experts/world,
 * uniform split, bootstrap.cuh:36-52); comms bootstrap itself lives on
 * the Python side (torch.distributed over RCCL). */
int fm_initialize(const fm_config* cfg, int rank, int world_size);

/* Replaces flashmoe::finalize (python_bindings.cu:163-168,
 * bootstrap.cuh:561-588): frees the workspace. */
int fm_finalize(void);

/* Router variant. fm_config describes the reference's
 * router: softmax over the E experts, plain top-k, combine weights
 * p_j / sum_selected p. This struct selects the routers of Qwen-MoE and
 * DeepSeek-V2/V3; every field defaults to the reference's behaviour. For
 * a token with fp32 logits l[e]:
 *   s[e] = softmax(l)[e] (scoring_func 0) | 1 / (1 + exp(-l[e])) (1)
 *   c[e] = s[e] + score_bias[e]           selection score; the bias never
 *                                         enters the weights
 *   groups: the E experts form n_group contiguous groups of E / n_group;
 *           a group's score is max c (group_score 0) or the sum of its two
 *           largest c (group_score 1); the topk_group best groups are kept
 *           (iterative strict-> first-index argmax) and only their experts
 *           can be selected. n_group 1 = no limit.
 *   top-k:  iterative strict-> first-index argmax over c, k times
 *   D     = (norm_topk_prob ? sum_j s[e_j] : 1.0f) / routed_scaling_factor
 * gate_out[t, :E] = Element(s), every tokenIds entry of the token carries
 * probSum = D, and the combine weight of selection j is Element(s[e_j]) / D.
 * Capacity, ordering and the shared-expert tail are those of the default.
 *
 * fm_set_router is valid after fm_initialize; fm_initialize and
 * fm_finalize reset the router to the defaults; NULL sets the defaults.
 * score_bias is BORROWED: the caller keeps it alive until the next
 * fm_set_router / fm_finalize and may rewrite its contents in place
 * between forwards. A set call invalidates the captured forward graph. A
 * non-default router always runs the multi-kernel path.
 * FM_ERR_UNSUPPORTED (the message names the key): num_experts not
 * divisible by n_group; n_group outside 1..16; topk_group outside
 * 1..n_group; expert_top_k > topk_group * E / n_group; group_score 1 with
 * fewer than 2 experts per group; routed_scaling_factor not finite or <= 0;
 * expert_top_k == 1 with norm_topk_prob 0 or a factor != 1 (the top-1
 * direct store is unscaled); is_training with any non-default field (the
 * aux-loss accumulators are softmax-specific); E > 256 with scoring_func 1,
 * a bias or n_group > 1 (norm_topk_prob and routed_scaling_factor alone
 * work at every E). */
typedef struct fm_router_config {
  int32_t scoring_func;          /* 0 softmax (default), 1 sigmoid */
  int32_t norm_topk_prob;        /* 1 (default) | 0 */
  int32_t n_group;               /* default 1 */
  int32_t topk_group;            /* default 1 */
  int32_t group_score;           /* 0 max (default), 1 sum of top 2 */
  float   routed_scaling_factor; /* default 1.0f */
  const float* score_bias;       /* device fp32 [E] or NULL; borrowed */
} fm_router_config;
int fm_set_router(const fm_router_config* r); /* NULL = defaults */
int fm_get_router(fm_router_config* out);

/* Weight scales of the fp8 expert weights (dtype 4 and 5; DESIGN.md
 * par.5l). Without them the weights are raw e4m3 with scale 1.0. With
 * granularity 1 every weight matrix row (output channel) r has an fp32 scale:
 *   W_eff[r, :] = float(W_fp8[r, :]) * s[r]
 * applied to the fp32 accumulator ahead of bias and activation:
 *   up, ungated  act(acc * s_up[p] + b_up[p])
 *   up, gated    act(g * s_glu[p]) * (u * s_up[p])
 *   down         acc * s_dn[h] + b_dn[h], then the combine as before
 * (dtype 5: the same; the in-epilogue activation quantisation sees the
 * scaled values). A per-tensor scale is the same value in every channel.
 * scales: device fp32, contiguous [nLx + nSh, SC], SC = P + H (+ P when
 * gated); an expert's record is [s_up (P) | s_dn (H) | s_glu (P)] - the slab
 * order - and the shared experts' records trail the routed ones. Every value
 * must be finite; the contents are not checked.
 * granularity: 0 none (scales ignored, may be NULL), 1 per output channel,
 * 2 reserved for 128x128 blocks -> FM_ERR_UNSUPPORTED.
 * Valid after fm_initialize; fm_initialize and fm_finalize reset to none.
 * The tensor is BORROWED until the next fm_set_weight_scales / fm_finalize;
 * the caller may rewrite its contents in place between forwards. A set call
 * invalidates the captured forward graph. Read by fm_moe_forward,
 * fm_moe_forward_phased, fm_expert_ffn, fm_expert_ffn_segments and
 * fm_expert_ffn_grouped (indexed by weight expert, like the bias slabs). A
 * forward with scales attached always runs the multi-kernel path
 * (fm_last_forward_fused() reports 0).
 * FM_ERR_UNSUPPORTED (the message names the cause): granularity 1 with a
 * torch_dtype other than 4 or 5; granularity 2. */
int fm_set_weight_scales(const float* scales, int32_t granularity);
int fm_get_weight_scales(const float** scales, int32_t* granularity);

/* Replaces _C.get_compiled_config (python_bindings.cu:170-183 /
 * flashmoe/ops.py:63-71): S, H, E, P, PX, element byte size. */
int fm_get_compiled_config(int64_t* S, int64_t* H, int64_t* E, int64_t* P,
                           int64_t* PX, int64_t* element_size);

/* Replaces _C.get_num_local_experts (python_bindings.cu:185-189). The
 * ROUTED local experts only: shared experts are not counted. */
int fm_get_num_local_experts(void);

/* num_shared_experts of the frozen config (-1 before fm_initialize). */
int fm_get_num_shared_experts(void);

/* 1 if the last fm_moe_forward / fm_moe_forward_phased ran the
 * single-launch fused kernel, 0 if it ran the multi-kernel path, -1
 * before fm_initialize. */
int fm_last_forward_fused(void);

/* 1 if the last fm_moe_forward / fm_moe_forward_phased ran its expert FFN on
 * the weight-streaming kernels of a decode-sized forward (k_decode_ffn), 0
 * if it ran the grouped GEMMs (always at S >= 128 and for fp32), -1 before
 * fm_initialize. */
int fm_last_forward_decode_ffn(void);

/* THE hot path. Replaces _C.moe_forward (python_bindings.cu:17-151) for
 * the single-rank case: gate -> route -> expert FFN -> combine on this
 * rank's tokens against this rank's nLx experts (world 1: all E).
 *
 * stream:    hipStream_t as void* (0 = default stream)
 * x:         [S, H] Element, device, contiguous
 * gate_w:    flat E*H Element buffer (the torch [H,E] tensor's storage,
 *            used as a row-major [E,H] matrix - reference quirk,
 *            moe.cuh:107-109; see oracle/moe_oracle.py docstring)
 * expert_w:  (nLx + num_shared_experts leading entries when the config
 *            has shared experts)
 *            [nLx, 2, P, H] Element ([e][0]=Wup [P,H]; [e][1] flat,
 *            used as [H,P] - moe.cuh:114-116); [nLx, 3, P, H] with
 *            [e][2]=Wglu [P,H] when hidden_act is gated (2/3)
 * b_up/b_dn: [nLx, P] / [nLx, H] Element or NULL (reference zero-fills,
 *            python_bindings.cu:80-82); b_up must be NULL when gated
 * gate_out:  [S, PX] Element out (softmax probs, moe.cuh:128-131)
 * moe_out:   [S, H] Element out
 * S:         token count this call (validated against frozen config)
 *
 * Asynchronous: enqueues on `stream`; no sync, no allocation. */
int fm_moe_forward(void* stream, const void* x, const void* gate_w,
                   const void* expert_w, const void* b_up, const void* b_dn,
                   void* gate_out, void* moe_out, int64_t S);

/* --- Staged entry points for the expert-parallel (multi-GPU) path.
 * The reference runs these stages inside one kernel with one-sided
 * NVSHMEM/P2P exchange between dispatch and FFN (moe.cuh:134-143); here
 * the host pipeline calls them around the RCCL all-to-all. --- */

/* Gate only: writes gate_out, and the library's tokenIds/eC workspace
 * (gate.cuh:474-720 semantics). */
int fm_gate_forward(void* stream, const void* x, const void* gate_w,
                    void* gate_out, int64_t S);

/* Copy routing results out: routed[e] = min(eC[e], EC) and the ordered
 * token slots (token index + probSum) per expert, for the host to build
 * the all-to-all. prob_sum is the token's combine denominator D of the
 * active router (fm_router_config: the sum of the selected scores by
 * default, 1 / routed_scaling_factor when norm_topk_prob is 0).
 * Device-to-host; synchronizes `stream`. */
int fm_read_routing(void* stream, uint32_t* routed_counts /* [E] */,
                    uint32_t* token_idx /* [E*EC] */,
                    float* prob_sum /* [E*EC] */);

/* Expert FFN on pre-packed rows (identity gather): rows [n_rows, H]
 * belong to local expert `local_e`; writes z = (act(rows@WupT+b))@WdnT+b
 * to out_rows [n_rows, H] (processor.cuh:685-751). Gated configs: the
 * gated h above, expert stride 3*P*H, b_up must be NULL (this holds for
 * fm_expert_ffn_segments / fm_expert_ffn_grouped too). */
int fm_expert_ffn(void* stream, const void* rows, const void* expert_w,
                  const void* b_up, const void* b_dn, void* out_rows,
                  int64_t n_rows, int32_t local_e);

/* --- Capacity-padded EP pipeline (the product multi-GPU path). The
 * exchange unit is the reference's symmetric-heap cell layout
 * (types.cuh:1014-1032): a fixed [E, EC, H] buffer, expert-major,
 * capacity-padded - so the all_to_all has STATIC equal splits and the
 * step needs no host synchronization at all. Rows past each expert's
 * routed count carry garbage and are dropped at the source. --- */

/* Gather x rows into the [E, EC, H] dispatch buffer per the last
 * fm_gate_forward's routing (os/packet.cuh:20-286 dispatch semantics). */
int fm_pack_dispatch(void* stream, const void* x, void* sendbuf);

/* FFN over the received padded buffer: rows = [n_segs, EC, H] with
 * seg_expert_dev = device int32[n_segs] mapping segment -> local expert
 * (canonical order: source-rank major). Two kernel launches total. */
int fm_expert_ffn_segments(void* stream, const void* rows,
                           const void* seg_expert_dev, int32_t n_segs,
                           const void* expert_w, void* out_rows);

/* Combine the returned [E, EC, H] buffer at the source using the local
 * routing metadata (scale = gate_out/probSum; k==1 unscaled) and write
 * moe_out (processor.cuh:44-205). */
int fm_combine_padded(void* stream, const void* returned,
                      const void* gate_out, void* moe_out, int64_t S);

/* Batched fm_expert_ffn over all local experts: rows are packed
 * expert-major; offsets = host array of n_experts+1 row offsets
 * (offsets[le]..offsets[le+1] belong to local expert le). One call per
 * EP step instead of nLx ctypes crossings. */
int fm_expert_ffn_grouped(void* stream, const void* rows,
                          const int64_t* offsets, int32_t n_experts,
                          const void* expert_w, const void* b_up,
                          const void* b_dn, void* out_rows);

/* Combine pre-scaled return rows into moe_out: for i < n_rows,
 * moe_out[token_idx[i]] += scale[i] * rows[i] (k>1 path,
 * processor.cuh:126-168); k==1: unscaled overwrite. Caller passes
 * scale[i] = gate_out[t,e]/probSum[t]. zero_first resets the fp32
 * accumulator before adding. finalize converts the accumulator into
 * moe_out. */
int fm_combine(void* stream, const void* rows, const uint32_t* token_idx,
               const float* scale, int64_t n_rows, int32_t zero_first);
int fm_combine_finalize(void* stream, void* moe_out, int64_t S);

/* Phase-timed variant of fm_moe_forward for roofline measurement
 * (replaces the reference's in-API benchmark loop semantics,
 * moe.cuh:146-184 forwardHostBench): HIP events are recorded between the
 * phases on `stream`, the stream is synchronized, and ms[0..3] receives
 * {gate, expert-up GEMM, expert-down GEMM+combine, other (memset/cast)}
 * durations in milliseconds. Not for use inside a timed region. */
int fm_moe_forward_phased(void* stream, const void* x, const void* gate_w,
                          const void* expert_w, const void* b_up,
                          const void* b_dn, void* gate_out, void* moe_out,
                          int64_t S, float ms[4]);

/* GPU-resident routing export for the EP pipeline: routed_dev = u32[E]
 * clipped counts (min(eC, EC)), tps_dev = u32[E][EC][2] (tokenIdx,
 * probSum bits). Device pointers; asynchronous (no host sync) - this is
 * what keeps the multi-GPU dispatch planning off the host critical path
 * (replaces the reference's in-kernel decode, os/packet.cuh:288-455). */
int fm_export_routing(void* stream, void* routed_dev, void* tps_dev);

/* --- Opt-in one-sided P2P transport for the EP exchange (the
 * reference's intra-node mode: direct stores into hipIpc-mapped peer
 * heap cells + system-scope 8-byte seq-tagged signals,
 * os/packet.cuh:214-258; heap cell layout = the padded pipeline's).
 * Enable from Python with FLASHMOE_P2P=1; the all_to_all path stays the
 * default until multi-GPU validation. --- */
int fm_heap_init(void);
int fm_heap_handle(void* out64 /* hipIpcMemHandle_t, 64 B */);
int fm_heap_connect(const void* handles /* world x 64 B; NULL = self only */);
int fm_heap_ptrs(void** recv /* [world,nLx,EC,H] */, void** ret /* [E,EC,H] */);
/* write routed rows into owners' heaps + signal; then wait for all
 * sources' cells for MY experts (bounded spin; prints on timeout) */
int fm_dispatch_p2p(void* stream, const void* x);
/* write FFN results back into sources' return heaps + signal; wait for
 * my own return cells */
int fm_return_p2p(void* stream, const void* ffn_out);
/* A timed-out in-kernel flag wait (bounded spin gave up) poisons the
 * exchange: the kernel sets a host-mapped error word, the NEXT
 * fm_dispatch_p2p/fm_return_p2p call returns FM_ERR_HIP without
 * launching, and this call checks definitively (synchronizes the
 * stream, returns FM_ERR_HIP if the word is set, then clears it so the
 * caller may retry). */
int fm_p2p_error_check(void* stream);

/* Training-mode auxiliary-loss accumulators (gate.cuh:273-299,763-773;
 * types.cuh:936-958): gML[e] = mean softmax prob of expert e over the
 * last forward's tokens, gMeC[e] = fraction routed to e (pre-capacity).
 * Host arrays of E floats; synchronizes the stream. is_training=1 only. */
int fm_read_aux_loss(void* stream, float* gML, float* gMeC);

/* Version/introspection */
const char* fm_last_error(void);
int fm_built_for_gfx950(void);

#ifdef __cplusplus
}
#endif
#endif /* FLASHMOE_ABI_H */
