// MI355X-native (gfx950 / CDNA4) implementation of the FlashDMoE hot path:
//   gate -> token routing -> grouped expert FFN (MFMA) -> weighted combine
// Built from scratch against the C-ABI in include/flashmoe_abi.h; semantics
// restated from the reference (citations per kernel, file:line into
// /root/reference). No CUDA compatibility paths; wave64 / MFMA / LDS only.
//
// Round-1 structure: separate kernels on one stream.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <type_traits>
#include <vector>

#include "../../include/flashmoe_abi.h"

// ---------------------------------------------------------------------------
// Common types / helpers
// ---------------------------------------------------------------------------

using bf16 = __hip_bfloat16;

// token slot descriptor (reference TPS, types.cuh:299-312): token index +
// sum of the token's selected top-k probabilities (gate.cuh:669,711-715).
// The top 4 bits of tokenIdx carry the assignment's position j within the
// token's top-k (tokens <= 2^28; lets the combine write non-atomic
// per-(token, j) slots instead of fp32 atomics).
struct __align__(8) TPS {
  uint32_t tokenIdx;
  float probSum;
};
__device__ __host__ __forceinline__ uint32_t tpsTok(uint32_t v) {
  return v & 0x0FFFFFFFu;
}
__device__ __host__ __forceinline__ uint32_t tpsJ(uint32_t v) { return v >> 28; }

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 halfx8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;

using fp16 = __half;
struct fp8e4m3 { uint8_t v; };  // storage-only; dequant at fragment read

// counted vmcnt wait with a compile-time literal (the triple-buffered
// staging pipeline waits for tile t+1 while t+2's glds stay in flight)
template <int N> __device__ __forceinline__ void wait_vmcnt() {
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
  else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if constexpr (N == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
  else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else static_assert(N == 0, "unsupported vmcnt literal");
}

typedef float f32x2n __attribute__((ext_vector_type(2)));
// convert 8 packed fp8-e4m3 (as 2 dwords) to 8 bf16 lanes - exact: every
// e4m3 value is bf16-representable (used at B fragment read, dtype 4)
__device__ __forceinline__ bf16x8 dequant_fp8x8_bf16(uint32_t lo, uint32_t hi) {
  bf16x8 r;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const uint32_t w = p ? hi : lo;
    const f32x2n f0 = __builtin_amdgcn_cvt_pk_f32_fp8(w, false);  // bytes 0,1
    const f32x2n f1 = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);   // bytes 2,3
    r[p * 4 + 0] = (__bf16)__float2bfloat16(f0.x);
    r[p * 4 + 1] = (__bf16)__float2bfloat16(f0.y);
    r[p * 4 + 2] = (__bf16)__float2bfloat16(f1.x);
    r[p * 4 + 3] = (__bf16)__float2bfloat16(f1.y);
  }
  return r;
}

// 2-byte element store, optionally agent-scope write-through (sc1) so
// same-launch consumers on other CUs/XCDs observe it without the
// producer issuing a cache-flushing release fence (Guideline 16 R1)
template <typename ET>
__device__ __forceinline__ void storeElem(ET* p, ET v, bool sc1) {
  if (sc1) {
    uint16_t b;
    __builtin_memcpy(&b, &v, 2);
    __hip_atomic_store(reinterpret_cast<uint16_t*>(p), b, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  } else {
    *p = v;
  }
}

__device__ __forceinline__ float toF(float v) { return v; }
__device__ __forceinline__ float toF(bf16 v) { return __bfloat162float(v); }
__device__ __forceinline__ float toF(fp16 v) { return __half2float(v); }
__device__ __forceinline__ void fromF(float v, float& o) { o = v; }
__device__ __forceinline__ void fromF(float v, bf16& o) { o = __float2bfloat16(v); }
__device__ __forceinline__ void fromF(float v, fp16& o) { o = __float2half(v); }

// element traits for the low-precision MFMA GEMM kernels (bf16 / fp16;
// both K=32 16x16 MFMA shapes share operand/result layouts on gfx950)
template <typename ET> struct ETr;
template <> struct ETr<bf16> {
  using vec8 = bf16x8;
  static __device__ __forceinline__ f32x4 mfma(vec8 a, vec8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ bf16 fromf(float v) { return __float2bfloat16(v); }
  // two conversions packed into one dword: ONE v_cvt_pk_bf16_f32 with
  // both sources (fromf compiles to the same instruction with one
  // source, so the rounding is identical)
  static __device__ __forceinline__ uint32_t pack2(float x, float y) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2v;
    const bf16x2v r = __builtin_convertvector(f32x2n{x, y}, bf16x2v);
    uint32_t w;
    __builtin_memcpy(&w, &r, 4);
    return w;
  }
};
template <> struct ETr<fp16> {
  using vec8 = halfx8;
  static __device__ __forceinline__ f32x4 mfma(vec8 a, vec8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ fp16 fromf(float v) { return __float2half(v); }
  static __device__ __forceinline__ uint32_t pack2(float x, float y) {
    typedef __attribute__((ext_vector_type(2))) _Float16 halfx2v;
    const halfx2v r = __builtin_convertvector(f32x2n{x, y}, halfx2v);
    uint32_t w;
    __builtin_memcpy(&w, &r, 4);
    return w;
  }
};

// hidden_act 0: ReLU, 1: exact-erf GELU (cutlass epilogue::thread::{ReLU,
// GELU}, schema csrc/flashmoe_config.schema.json:33-37, types.cuh:151-159)
// - applied inline in the GEMM epilogues via the compile-time ACT param.

#define DIVUP(a, b) (((a) + (b) - 1) / (b))

// ---------------------------------------------------------------------------
// Split gate (v2): the single-kernel gate ran on only S/128 blocks (32 for
// config 2 - 12% of the CUs, 61% wave-park, profiles/r01). k_gate_logits
// parallelises the logit GEMM over (token-tile, H-chunk) blocks with fp32
// atomicAdd partials into a global logits buffer; k_gate_route then does
// softmax/top-k/ordering per token tile (same semantics as k_gate,
// gate.cuh:474-720).
// ---------------------------------------------------------------------------

// TAIL (decode-sized forwards, S < 128): rows >= S of the
// one tile are neither read from x nor accumulated into logits32.
template <typename T, bool TAIL = false>
__global__ __launch_bounds__(256) void k_gate_logits(
    const T* __restrict__ x, const T* __restrict__ gate_w,
    float* __restrict__ logits32, uint32_t* __restrict__ eC, int S, int H,
    int E, int Hc) {
  // fold the eC zeroing into the first block (route runs after this
  // kernel; saves a 4-us launch-bound memset per forward)
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
    for (int i = threadIdx.x; i < E; i += blockDim.x) eC[i] = 0;
  }
  // blockIdx.z selects a chunk of <=128 experts (E up to 256, config 5)
  const int eBase = blockIdx.z * 128;
  const int Ec = min(E - eBase, 128);
  constexpr int BM = 128;
  constexpr int BK = 64;
  constexpr int RPAD = 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* part = reinterpret_cast<float*>(smem);          // [BM][Ec+1]
  T* aCh = nullptr;  // assigned after Ec is known (see below)
  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * BM;
  const int tok = tid & (BM - 1);
  const int half = tid >> 7;
  const int E2 = (Ec + 1) / 2;
  const int e0 = half * E2;
  const int e1 = min(e0 + E2, Ec);
  const int k0 = blockIdx.y * Hc;
  const int k1 = min(H, k0 + Hc);
  aCh = reinterpret_cast<T*>(part + BM * (Ec + 1));      // [BM][BK+RPAD]
  const int LDA = BK + RPAD;
  T* gCh = aCh + BM * LDA;                               // [Ec][BK+RPAD]

  for (int i = tid; i < BM * (Ec + 1); i += 256) part[i] = 0.0f;
  for (int kc = k0; kc < k1; kc += BK) {
    constexpr int EPU = 16 / sizeof(T);
    {
      const int unitsA = BM * BK / EPU;
      for (int u = tid; u < unitsA; u += 256) {
        const int row = u / (BK / EPU);
        const int cu = u % (BK / EPU);
        if constexpr (TAIL) {
          if (m0 + row >= S) {
            *reinterpret_cast<u32x4*>(aCh + row * LDA + cu * EPU) =
                u32x4{0u, 0u, 0u, 0u};
            continue;
          }
        }
        *reinterpret_cast<u32x4*>(aCh + row * LDA + cu * EPU) =
            *reinterpret_cast<const u32x4*>(x + (size_t)(m0 + row) * H + kc + cu * EPU);
      }
      const int unitsG = Ec * BK / EPU;
      for (int u = tid; u < unitsG; u += 256) {
        const int row = u / (BK / EPU);
        const int cu = u % (BK / EPU);
        *reinterpret_cast<u32x4*>(gCh + row * LDA + cu * EPU) =
            *reinterpret_cast<const u32x4*>(gate_w + (size_t)(eBase + row) * H +
                                            kc + cu * EPU);
      }
    }
    __syncthreads();
    const T* arow = aCh + tok * LDA;
    u32x4 a8[BK * sizeof(T) / 16];
#pragma unroll
    for (int jb = 0; jb < BK * (int)sizeof(T) / 16; ++jb)
      a8[jb] = *reinterpret_cast<const u32x4*>(&arow[jb * (16 / sizeof(T))]);
    for (int e = e0; e < e1; ++e) {
      const T* grow = gCh + e * LDA;
      float sAcc = 0.0f;
#pragma unroll
      for (int jb = 0; jb < BK * (int)sizeof(T) / 16; ++jb) {
        const u32x4 g8 = *reinterpret_cast<const u32x4*>(&grow[jb * (16 / sizeof(T))]);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const uint32_t aw = a8[jb][w], gw = g8[w];
          if constexpr (__is_same(T, bf16)) {
            const float2 av = __bfloat1622float2(
                *reinterpret_cast<const __hip_bfloat162*>(&aw));
            const float2 gv = __bfloat1622float2(
                *reinterpret_cast<const __hip_bfloat162*>(&gw));
            sAcc = fmaf(av.x, gv.x, sAcc);
            sAcc = fmaf(av.y, gv.y, sAcc);
          } else if constexpr (__is_same(T, fp16)) {
            const float2 av = __half22float2(*reinterpret_cast<const __half2*>(&aw));
            const float2 gv = __half22float2(*reinterpret_cast<const __half2*>(&gw));
            sAcc = fmaf(av.x, gv.x, sAcc);
            sAcc = fmaf(av.y, gv.y, sAcc);
          } else {
            sAcc = fmaf(__uint_as_float(aw), __uint_as_float(gw), sAcc);
          }
        }
      }
      part[tok * (Ec + 1) + e] += sAcc;
    }
    __syncthreads();
  }
  // one atomic per (token, expert) per H-chunk
  if constexpr (TAIL) {
    if (m0 + tok >= S) return;
  }
  for (int e = e0; e < e1; ++e)
    atomicAdd(logits32 + (size_t)(m0 + tok) * E + eBase + e,
              part[tok * (Ec + 1) + e]);
}

// ---------------------------------------------------------------------------
// Softmax / top-k / ordered placement for one 128-token tile (reference
// gate.cuh:557-718 semantics): the shared core of k_gate_route (classic
// path) and the fused kernel's inline route. 512 threads; the per-token
// top-k runs on FOUR threads per token, each owning a <=64-expert chunk
// with a u64 taken-mask and combining candidates with width-4 shuffles
// (larger value wins, equal value -> smaller index == the reference's
// ascending strict-> first-index scan). The serial one-thread-per-token
// scan was the dominant gate cost at E=256 (~144 us at the cfg5 shape).
// Reads the tile's logits from logits32 and RE-ZEROES them (keeps the
// split-K logits accumulate memset-free).
// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// Router variants (fm_router_config): sigmoid scoring, a
// selection bias, group-limited top-k, unnormalised / scaled weights. Both
// gates compile them behind the template switch RV; the RV = false
// instantiations are the legacy code, untouched. In an RV instantiation
// the token's LDS logits row is rewritten IN PLACE with the scores s (no
// second tile: 128 x (E + 1) x 4 B is 131 KB at E = 256), the selection
// score c[e] = row[e] + sB[e] is formed in the scan from an LDS copy of the
// bias (zeros without one), and the group limit enters as the initial
// taken-mask, so the scan itself has no new branch. selLogits (softmax, no
// bias, group_score 0): c is monotone in the logits, so the row keeps the
// logits and selection, mCw and gate_out are computed exactly as the legacy
// code computes them - a pure norm / factor variant selects bit-identically
// to the default router.
// ---------------------------------------------------------------------------
struct RouterP {
  const float* bias;  // device fp32 [E] or null
  float factor;       // routed_scaling_factor
  int scoring, norm, G, TG, gscore;
  int selLogits;      // scoring 0 && !bias && gscore 0
};

constexpr int kMaxGroups = 16;

// scores of one thread's chunk [e0, e1) of a token row; SUBS threads per
// token. Softmax: m / inv_d by the legacy reduction order. Returns with the
// row holding s (or still the logits when selLogits).
__device__ __forceinline__ void rv_scores(float* lrow, int e0, int e1,
                                          int SUBS, const RouterP& rp,
                                          float& m, float& inv_d) {
  m = 0.0f;
  inv_d = 1.0f;
  if (rp.scoring == 0) {
    m = -INFINITY;
    for (int e = e0; e < e1; ++e) m = fmaxf(m, lrow[e]);
    for (int off = 1; off < SUBS; off <<= 1)
      m = fmaxf(m, __shfl_xor(m, off, SUBS));
    float d = 0.0f;
    for (int e = e0; e < e1; ++e) d += __expf(lrow[e] - m);
    for (int off = 1; off < SUBS; off <<= 1) d += __shfl_xor(d, off, SUBS);
    inv_d = 1.0f / d;
    if (!rp.selLogits)
      for (int e = e0; e < e1; ++e) lrow[e] = __expf(lrow[e] - m) * inv_d;
  } else {
    for (int e = e0; e < e1; ++e) lrow[e] = 1.0f / (1.0f + __expf(-lrow[e]));
  }
}

// group scores of the groups sub, sub + SUBS, ... of one token: max c, or
// the sum of the two largest c (other threads' chunks: after a barrier)
__device__ __forceinline__ void rv_group_scores(const float* lrow,
                                                const float* sB, float* sGrow,
                                                int sub, int SUBS, int E,
                                                const RouterP& rp) {
  const int gs = E / rp.G;
  for (int gi = sub; gi < rp.G; gi += SUBS) {
    float a = -INFINITY, b = -INFINITY;  // largest, second largest
    for (int e = gi * gs; e < (gi + 1) * gs; ++e) {
      const float c = lrow[e] + sB[e];
      if (c > a) { b = a; a = c; }
      else if (c > b) b = c;
    }
    sGrow[gi] = rp.gscore ? a + b : a;
  }
}

// initial taken-mask of the chunk [e0, e1): the experts outside the TG best
// groups (strict-> first-index argmax, TG times). Every thread of the token
// computes the same kept set from the same LDS group scores.
__device__ __forceinline__ unsigned long long rv_group_taken(
    const float* sGrow, int e0, int e1, int E, const RouterP& rp) {
  uint32_t keepG = 0u;
  for (int i = 0; i < rp.TG; ++i) {
    float bv = -INFINITY;
    int bi = -1;
    for (int gi = 0; gi < rp.G; ++gi) {
      const float v = sGrow[gi];
      if (!((keepG >> gi) & 1u) && v > bv) { bv = v; bi = gi; }
    }
    if (bi >= 0) keepG |= 1u << bi;
  }
  const int gs = E / rp.G;
  unsigned long long taken = 0ull;
  for (int e = e0; e < e1; ++e)
    if (!((keepG >> (e / gs)) & 1u)) taken |= 1ull << (e - e0);
  return taken;
}

// TAIL (decode-sized forwards, S < 128): the tile is
// ragged. A row >= S is not read from logits32, selects the sentinel E in
// every slot (the counting scan never counts it, so it adds nothing to eC)
// and writes no gate_out row, kept entry or tokenIds entry. TAIL = false
// compiles to the code it was.
template <typename T, int K, bool RV = false, bool TAIL = false>
__device__ __forceinline__ void route_tile_core(
    char* smem, float* __restrict__ logits32, T* __restrict__ gate_out,
    TPS* __restrict__ tokenIds, uint32_t* __restrict__ eC,
    uint8_t* __restrict__ kept, float* __restrict__ gML,
    float* __restrict__ gMeC, int S, int E, int PX, int EC, int pEC,
    int m0, const RouterP& rp = RouterP{}) {
  // TT tokens per pass: 128 normally; 64 half-passes at E > 256 so the
  // fp32 logits tile fits LDS (64 x 513 x 4 B = 131 KB at E = 512).
  // SUBS = 512/TT threads cooperate per token (chunk <= 64 experts each,
  // so the taken-mask stays one u64). Pass order preserves token order,
  // so intra-tile placement semantics are unchanged.
  const int TT = (E > 256) ? 64 : 128;
  const int SUBS = 512 / TT;
  float* logits = reinterpret_cast<float*>(smem);                  // [TT][E+1]
  uint16_t* sel = reinterpret_cast<uint16_t*>(logits + TT * (E + 1));
  uint16_t* localIdx = sel + TT * K;
  // +2: one dump slot so the counting scan's store is UNCONDITIONAL
  // (an exec-masked conditional store compiled into ~520 serial
  // s_and_saveexec blocks = ~80% of the round-1 kernel's runtime)
  uint32_t* base = reinterpret_cast<uint32_t*>(localIdx + TT * K + 2);  // [E]
  float* sInv = reinterpret_cast<float*>(base + E);                // [TT] 1/d
  float* sMax = sInv + TT;                                         // [TT]
  float* sCw = sMax + TT;                                          // [TT] mCw
  float* sB = sCw + TT;             // RV only: [E] selection bias
  float* sGrp = sB + E;             // RV only: [TT][kMaxGroups] group scores
  const int tid = threadIdx.x;
  for (int pass = 0; pass < 128 / TT; ++pass) {
  const int pm0 = m0 + pass * TT;
  __syncthreads();  // prior pass's LDS readers done
  for (int i = tid; i < TT * E; i += 512) {
    const int row = i / E, col = i % E;
    if constexpr (TAIL) {
      if (pm0 + row >= S) {  // finite filler: the row's selections are void
        logits[row * (E + 1) + col] = 0.0f;
        continue;
      }
    }
    float* src = &logits32[(size_t)(pm0 + row) * E + col];
    logits[row * (E + 1) + col] = *src;
    *src = 0.0f;
  }
  if constexpr (RV)
    for (int e = tid; e < E; e += 512) sB[e] = rp.bias ? rp.bias[e] : 0.0f;
  __syncthreads();

  if constexpr (RV) {
    // 512 = TT * SUBS threads: every thread owns a (token, chunk), so the
    // barriers below are reached by all of them
    const int token = tid / SUBS;
    const int sub = tid % SUBS;
    float* lrow = logits + token * (E + 1);
    const int chunk = (E + SUBS - 1) / SUBS;  // <= 64: u64 taken-mask
    const int e0 = min(E, sub * chunk);
    const int e1 = min(E, e0 + chunk);
    float m, inv_d;
    rv_scores(lrow, e0, e1, SUBS, rp, m, inv_d);
    if (sub == 0) {
      sInv[token] = inv_d;  // read by the gate_out pass when selLogits
      sMax[token] = m;
    }
    __syncthreads();  // rows hold s: group scores read other chunks
    if (rp.G > 1)
      rv_group_scores(lrow, sB, sGrp + token * kMaxGroups, sub, SUBS, E, rp);
    __syncthreads();
    unsigned long long takenM =
        rp.G > 1 ? rv_group_taken(sGrp + token * kMaxGroups, e0, e1, E, rp)
                 : 0ull;
    float mCw = 0.0f;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      float lv = -INFINITY;
      int li = E;  // sentinel sorts after every real index
      for (int e = e0; e < e1; ++e) {
        const bool tk = (takenM >> (e - e0)) & 1ull;
        const float c = lrow[e] + sB[e];
        if (!tk && c > lv) { lv = c; li = e; }
      }
      for (int off = 1; off < SUBS; off <<= 1) {
        const float ov = __shfl_xor(lv, off, SUBS);
        const int oi = __shfl_xor(li, off, SUBS);
        if (ov > lv || (ov == lv && oi < li)) { lv = ov; li = oi; }
      }
      if (li >= e0 && li < e1) takenM |= 1ull << (li - e0);
      if (sub == 0) {
        sel[token * K + i] =
            (TAIL && pm0 + token >= S) ? (uint16_t)E : (uint16_t)li;
        if (rp.selLogits) mCw += __expf(lv - m) * inv_d;
        else if (li < E) mCw += lrow[li];
      }
    }
    if (sub == 0) sCw[token] = (rp.norm ? mCw : 1.0f) / rp.factor;
  } else {
    const int token = tid / SUBS;
    const int sub = tid % SUBS;
    if (token < TT) {
      const float* lrow = logits + token * (E + 1);
      const int chunk = (E + SUBS - 1) / SUBS;  // <= 64: u64 taken-mask
      const int e0 = sub * chunk;
      const int e1 = min(E, e0 + chunk);
      float m = -INFINITY;
      for (int e = e0; e < e1; ++e) m = fmaxf(m, lrow[e]);
#pragma unroll
      for (int off = 1; off < 8; off <<= 1)
        if (off < SUBS) m = fmaxf(m, __shfl_xor(m, off, SUBS));
      float d = 0.0f;
      for (int e = e0; e < e1; ++e) d += __expf(lrow[e] - m);
#pragma unroll
      for (int off = 1; off < 8; off <<= 1)
        if (off < SUBS) d += __shfl_xor(d, off, SUBS);
      const float inv_d = 1.0f / d;
      if (sub == 0) {
        sInv[token] = inv_d;  // the coalesced gate_out pass below
        sMax[token] = m;      // recomputes probs from these
      }
      unsigned long long takenM = 0ull;
      float mCw = 0.0f;
#pragma unroll
      for (int i = 0; i < K; ++i) {
        float lv = -INFINITY;
        int li = E;  // sentinel sorts after every real index
        for (int e = e0; e < e1; ++e) {
          const bool tk = (takenM >> (e - e0)) & 1ull;
          if (!tk && lrow[e] > lv) { lv = lrow[e]; li = e; }
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
          if (off < SUBS) {
            const float ov = __shfl_xor(lv, off, SUBS);
            const int oi = __shfl_xor(li, off, SUBS);
            if (ov > lv || (ov == lv && oi < li)) { lv = ov; li = oi; }
          }
        }
        if (li >= e0 && li < e1) takenM |= 1ull << (li - e0);
        if (sub == 0) {
          sel[token * K + i] =
              (TAIL && pm0 + token >= S) ? (uint16_t)E : (uint16_t)li;
          mCw += __expf(lv - m) * inv_d;
        }
      }
      if (sub == 0) sCw[token] = mCw;
    }
  }
  __syncthreads();
  // cooperative COALESCED gate_out store (recompute probs from LDS; a
  // per-token scalar store pattern was one cache line per element)
  for (int i = tid * 8; i < TT * PX; i += 512 * 8) {
    const int row = i / PX, col0 = i % PX;
    if constexpr (TAIL) {
      if (pm0 + row >= S) continue;
    }
    const float mR = sMax[row], ivR = sInv[row];
    const float* lrow = logits + row * (E + 1);
    struct __attribute__((aligned(16))) V8 { T x[8]; } v;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int col = col0 + q;
      float pv;
      if constexpr (RV)  // the row already holds s unless selLogits
        pv = (col < E) ? (rp.selLogits ? __expf(lrow[col] - mR) * ivR
                                       : lrow[col])
                       : 0.0f;
      else
        pv = (col < E) ? __expf(lrow[col] - mR) * ivR : 0.0f;
      fromF(pv, v.x[q]);
    }
    *reinterpret_cast<V8*>(gate_out + (size_t)(pm0 + row) * PX + col0) = v;
  }
  __syncthreads();
  if (tid < E) {
    // 16-B LDS reads, 8 selections per iteration (a scalar dependent
    // scan exposed ~50 cycles of LDS latency per entry: ~7 us/fwd)
    uint32_t cnt = 0;
    for (int mj = 0; mj < TT * K; mj += 8) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(sel + mj);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const uint32_t w = v[q >> 1];
        const uint16_t sv = (q & 1) ? (uint16_t)(w >> 16) : (uint16_t)(w & 0xffff);
        const bool mt = (sv == (uint16_t)tid);
        localIdx[mt ? (mj + q) : TT * K] = (uint16_t)cnt;
        cnt += mt;
      }
    }
    base[tid] = __hip_atomic_fetch_add(eC + tid, cnt, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
    if (gML) {
      // column sum of probs for this expert over the pass's tokens
      float colSum = 0.0f;
      for (int mj = 0; mj < TT; ++mj)
        colSum += __expf(logits[mj * (E + 1) + tid] - sMax[mj]) * sInv[mj];
      atomicAdd(gML + tid, colSum / (float)S);
      atomicAdd(gMeC + tid, (float)cnt / (float)S);
    }
  }
  __syncthreads();
  if (tid < TT && (!TAIL || pm0 + tid < S)) {
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const int e = sel[tid * K + i];
      if constexpr (RV) {
        // e == E: no selectable expert was left (a bias of -inf or NaN
        // scores); the slot is dropped, never indexed
        if (e >= E) {
          if (kept) kept[(size_t)(pm0 + tid) * K + i] = 0;
          continue;
        }
      }
      const uint32_t slot = base[e] + localIdx[tid * K + i];
      const bool keep = slot < (uint32_t)EC;
      if (keep) {
        tokenIds[(size_t)e * pEC + slot] =
            TPS{(uint32_t)(pm0 + tid) | ((uint32_t)i << 28), sCw[tid]};
      }
      if (kept) kept[(size_t)(pm0 + tid) * K + i] = keep ? 1 : 0;
    }
  }
  }  // pass loop
}

template <typename T, int K, bool RV = false, bool TAIL = false>
__global__ __launch_bounds__(512) void k_gate_route(
    float* __restrict__ logits32, T* __restrict__ gate_out,
    TPS* __restrict__ tokenIds, uint32_t* __restrict__ eC, int S, int E,
    int PX, int EC, int pEC, float* __restrict__ gML,
    float* __restrict__ gMeC, uint8_t* __restrict__ kept, RouterP rp) {
  // gML/gMeC: training-mode aux-loss accumulators (gate.cuh:273-299,
  // 763-773; types.cuh:936-958). Null in inference mode.
  // rp: read by the RV instantiations only
  extern __shared__ __attribute__((aligned(16))) char smem[];
  route_tile_core<T, K, RV, TAIL>(smem, logits32, gate_out, tokenIds, eC, kept,
                                  gML, gMeC, S, E, PX, EC, pEC,
                                  blockIdx.x * 128, rp);
}

// ---------------------------------------------------------------------------
// Single-launch deterministic gate (bf16/fp16, E <= 64, inference):
// grid = (S/128 tiles) x (128/TB sub-blocks). Each sub-block computes the
// logits of its TB tokens with MFMA over the WHOLE K = H (K split over
// four waves in contiguous ranges that depend on H alone, partials summed
// through LDS in wave order -> the logits are a pure function of the
// inputs, no atomics), then softmax / top-k exactly as route_tile_core,
// stores its gate_out rows and hands sel / mCw to the tile's LAST
// arriving sub-block through global scratch (producer half of the
// Guideline 16 hand-off in its write-through form, R1: the payload is
// stored sc1 like storeElem's, so the ticket needs no cache-flushing
// release fence - the fenced form measured 3.4 us slower per launch,
// DESIGN.md par.5g). The last arriver places the tile's 128 x K
// selections (ballot + prefix popcount per expert, token order inside the
// tile, one fetch_add per expert between tiles - the k_gate_route
// semantics). No block ever waits for another: no spin, no co-residency
// requirement. All ticket words are left zero for the next launch.
// ---------------------------------------------------------------------------

// arrive on a ticket word: every wave drains its stores (write-through
// payload) and returning atomics, then thread 0 takes the ticket; every
// thread gets the ticket's prior value. When it equals lastVal the block
// is the last arriver and thread 0 also issues the (single) agent-scope
// acquire. Everything handed over through a ticket is either stored sc1
// (sel, mCw) or an agent-scope atomic (eCacc).
__device__ __forceinline__ uint32_t gate_arrive(uint32_t* ctr,
                                                uint32_t lastVal,
                                                uint32_t* sFlag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t old = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
    if (old == lastVal) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    *sFlag = old;
  }
  __syncthreads();
  return *sFlag;
}

// U K-steps of 32: all U (1 + NE) fragment loads issue before the first
// MFMA waits (the kernel is latency-bound, not issue-bound; at H = 1024 a
// wave's whole K range is one trip of 8 - which measured the same as two
// trips of 4)
template <typename T, int NE, int U>
__device__ __forceinline__ void gate_logits_trip(const T* __restrict__ xrow,
                                                 const T* const (&wp)[NE],
                                                 int s, f32x4 (&acc)[4]) {
  using vec8 = typename ETr<T>::vec8;
  vec8 xv[U], wv[U][NE];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    xv[u] = *reinterpret_cast<const vec8*>(xrow + (s + u) * 32);
#pragma unroll
    for (int f = 0; f < NE; ++f)
      wv[u][f] = *reinterpret_cast<const vec8*>(wp[f] + (s + u) * 32);
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int f = 0; f < NE; ++f)
      acc[f] = ETr<T>::mfma(wv[u][f], xv[u], acc[f]);
}

// one wave's share of the logits: 16 token rows x (NE x 16) expert columns
// over K steps [s0, s1) of 32. Operand fragments go straight from global
// to registers (16 B per lane; no other wave shares them). Swapped
// operands as in gemm_job_body: lane & 15 = token row, acc[f][0..3] =
// expert columns 16 f + 4 (lane >> 4) + 0..3.
template <typename T, int NE>
__device__ __forceinline__ void gate_logits_wave(const T* __restrict__ xrow,
                                                 const T* __restrict__ gate_w,
                                                 int H, int E, int lane,
                                                 int s0, int s1,
                                                 f32x4 (&acc)[4]) {
  const T* wp[NE];
#pragma unroll
  for (int f = 0; f < NE; ++f)
    wp[f] = gate_w + (size_t)min(f * 16 + (lane & 15), E - 1) * H +
            (lane >> 4) * 8;
  int s = s0;
  for (; s + 8 <= s1; s += 8) gate_logits_trip<T, NE, 8>(xrow, wp, s, acc);
  if (s + 4 <= s1) { gate_logits_trip<T, NE, 4>(xrow, wp, s, acc); s += 4; }
  for (; s < s1; ++s) gate_logits_trip<T, NE, 1>(xrow, wp, s, acc);
}

// -DFM_GEMM_STAMPS (measurement build only): thread 0 of every block of
// k_gate_fused (slot 0) and k_cast_combine (slot 1) records the 100 MHz
// wall clock at entry and exit, so tools/gemm_phase_stamps.py can lay the
// four kernels of a forward on one timeline (see g_gemmStamps below).
#ifdef FM_GEMM_STAMPS
constexpr int FM_AUX_KERNELS = 2, FM_AUX_BLOCKS = 4096;
__device__ unsigned long long g_auxStamps[FM_AUX_KERNELS][FM_AUX_BLOCKS][2];
#define FM_AUX_STAMP(k, i)                                                    \
  do {                                                                        \
    if (threadIdx.x == 0 && blockIdx.x < FM_AUX_BLOCKS)                       \
      g_auxStamps[k][blockIdx.x][i] = __builtin_amdgcn_s_memrealtime();       \
  } while (0)
#else
#define FM_AUX_STAMP(k, i) do {} while (0)
#endif

template <typename T, int K, int TB, bool RV = false>
__global__ __launch_bounds__(TB * 16) void k_gate_fused(
    const T* __restrict__ x, const T* __restrict__ gate_w,
    T* __restrict__ gate_out, uint16_t* gateSel, float* gateCw,
    uint32_t* tilesDone, uint32_t* tileArrive, uint32_t* eCacc,
    TPS* __restrict__ tokenIds, uint32_t* __restrict__ eC,
    uint8_t* __restrict__ kept, int H, int E, int PX, int EC, int pEC,
    RouterP rp /* read by the RV instantiations only */) {
  constexpr int NT = TB * 16;    // threads
  constexpr int NWV = NT / 64;   // waves: TB/16 row groups x 4 K ranges
  constexpr int SUB = 128 / TB;  // sub-blocks per tile
  constexpr int LDP = 68;        // partial row stride (16-B aligned rows)
  constexpr int LDL = 65;        // logits row stride (E <= 64)
  __shared__ __attribute__((aligned(16))) float part[NWV * 16 * LDP];
  __shared__ float logits[TB * LDL];
  __shared__ float sInv[TB], sMax[TB];
  __shared__ __attribute__((aligned(16))) uint16_t sSel[128 * K];
  __shared__ uint16_t sLoc[128 * K];
  __shared__ float sCw[128];
  __shared__ uint32_t cntH[2 * 64];
  __shared__ uint32_t base[64];
  __shared__ uint32_t sFlag[2];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  FM_AUX_STAMP(0, 0);
  const int tile = blockIdx.x / SUB;
  const int m0 = blockIdx.x * TB;  // first token of this sub-block

  // ---- logits: whole K inside the block -----------------------------
  {
    const int kSteps = H / 32;
    const int spw = DIVUP(kSteps, 4);
    const int ks = wave & 3, rg = wave >> 2;
    const int s0 = min(ks * spw, kSteps);
    const int s1 = min(s0 + spw, kSteps);
    f32x4 acc[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
    const T* xrow =
        x + (size_t)(m0 + rg * 16 + (lane & 15)) * H + (lane >> 4) * 8;
    const int NEr = DIVUP(E, 16);
    if (NEr == 1) gate_logits_wave<T, 1>(xrow, gate_w, H, E, lane, s0, s1, acc);
    else if (NEr == 2) gate_logits_wave<T, 2>(xrow, gate_w, H, E, lane, s0, s1, acc);
    else gate_logits_wave<T, 4>(xrow, gate_w, H, E, lane, s0, s1, acc);
    float* prow = part + (wave * 16 + (lane & 15)) * LDP + (lane >> 4) * 4;
#pragma unroll
    for (int f = 0; f < 4; ++f)
      if (f < NEr) *reinterpret_cast<f32x4*>(prow + f * 16) = acc[f];
  }
  __syncthreads();
  // fixed wave-order reduction of the four K-range partials
  for (int i = tid; i < TB * E; i += NT) {
    const int row = i / E, col = i % E;
    const float* p = part + ((row >> 4) * 4 * 16 + (row & 15)) * LDP + col;
    float v = p[0];
    v += p[16 * LDP];
    v += p[2 * 16 * LDP];
    v += p[3 * 16 * LDP];
    logits[row * LDL + col] = v;
  }
  __syncthreads();

  // ---- softmax / top-k: four threads per token (route_tile_core) -----
  if constexpr (RV) {
    // router variant: scores in place, group scores through LDS, group
    // limit as the initial taken-mask (see RouterP). The two barriers are
    // outside the tid test; mCw in the hand-off payload carries D.
    constexpr int SUBS = 4;
    __shared__ float sB[64];
    __shared__ float sGrp[TB * kMaxGroups];
    const bool act = tid < TB * 4;
    const int token = act ? tid / SUBS : 0;
    const int sub = tid % SUBS;
    float* lrow = logits + token * LDL;
    const int chunk = (E + SUBS - 1) / SUBS;
    const int e0 = min(E, sub * chunk);
    const int e1 = min(E, e0 + chunk);
    float m = 0.0f, inv_d = 1.0f;
    if (tid >= NT - 64 && lane < E)  // the last wave: idle until the barrier
      sB[lane] = rp.bias ? rp.bias[lane] : 0.0f;
    if (act) {
      rv_scores(lrow, e0, e1, SUBS, rp, m, inv_d);
      if (sub == 0) {
        sInv[token] = inv_d;
        sMax[token] = m;
      }
    }
    __syncthreads();
    if (act && rp.G > 1)
      rv_group_scores(lrow, sB, sGrp + token * kMaxGroups, sub, SUBS, E, rp);
    __syncthreads();
    if (act) {
      uint32_t takenM =  // chunk <= 16
          rp.G > 1 ? (uint32_t)rv_group_taken(sGrp + token * kMaxGroups, e0,
                                              e1, E, rp)
                   : 0u;
      float mCw = 0.0f;
#pragma unroll
      for (int i = 0; i < K; ++i) {
        float lv = -INFINITY;
        int li = E;  // sentinel sorts after every real index
        for (int e = e0; e < e1; ++e) {
          const bool tk = (takenM >> (e - e0)) & 1u;
          const float c = lrow[e] + sB[e];
          if (!tk && c > lv) { lv = c; li = e; }
        }
#pragma unroll
        for (int off = 1; off < SUBS; off <<= 1) {
          const float ov = __shfl_xor(lv, off, SUBS);
          const int oi = __shfl_xor(li, off, SUBS);
          if (ov > lv || (ov == lv && oi < li)) { lv = ov; li = oi; }
        }
        if (li >= e0 && li < e1) takenM |= 1u << (li - e0);
        if (sub == 0) {
          __hip_atomic_store(gateSel + (size_t)(m0 + token) * K + i,
                             (uint16_t)li, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
          if (rp.selLogits) mCw += __expf(lv - m) * inv_d;
          else if (li < E) mCw += lrow[li];
        }
      }
      if (sub == 0)
        __hip_atomic_store(gateCw + m0 + token,
                           (rp.norm ? mCw : 1.0f) / rp.factor,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  } else if (tid < TB * 4) {
    constexpr int SUBS = 4;
    const int token = tid / SUBS;
    const int sub = tid % SUBS;
    const float* lrow = logits + token * LDL;
    const int chunk = (E + SUBS - 1) / SUBS;
    const int e0 = min(E, sub * chunk);
    const int e1 = min(E, e0 + chunk);
    float m = -INFINITY;
    for (int e = e0; e < e1; ++e) m = fmaxf(m, lrow[e]);
#pragma unroll
    for (int off = 1; off < SUBS; off <<= 1)
      m = fmaxf(m, __shfl_xor(m, off, SUBS));
    float d = 0.0f;
    for (int e = e0; e < e1; ++e) d += __expf(lrow[e] - m);
#pragma unroll
    for (int off = 1; off < SUBS; off <<= 1) d += __shfl_xor(d, off, SUBS);
    const float inv_d = 1.0f / d;
    if (sub == 0) {
      sInv[token] = inv_d;
      sMax[token] = m;
    }
    uint32_t takenM = 0u;  // chunk <= 16
    float mCw = 0.0f;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      float lv = -INFINITY;
      int li = E;  // sentinel sorts after every real index
      for (int e = e0; e < e1; ++e) {
        const bool tk = (takenM >> (e - e0)) & 1u;
        if (!tk && lrow[e] > lv) { lv = lrow[e]; li = e; }
      }
#pragma unroll
      for (int off = 1; off < SUBS; off <<= 1) {
        const float ov = __shfl_xor(lv, off, SUBS);
        const int oi = __shfl_xor(li, off, SUBS);
        if (ov > lv || (ov == lv && oi < li)) { lv = ov; li = oi; }
      }
      if (li >= e0 && li < e1) takenM |= 1u << (li - e0);
      if (sub == 0) {
        __hip_atomic_store(gateSel + (size_t)(m0 + token) * K + i,
                           (uint16_t)li, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        mCw += __expf(lv - m) * inv_d;
      }
    }
    if (sub == 0)
      __hip_atomic_store(gateCw + m0 + token, mCw, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
  // ---- arrive as soon as the hand-off payload is out: the gate_out rows
  // below are not part of it, so they stay off the last arriver's critical
  // path (the arrive's barriers also order sMax / sInv for them)
  const bool lastOfTile =
      gate_arrive(tileArrive + tile, SUB - 1, &sFlag[0]) == SUB - 1;
  // coalesced gate_out rows [TB, PX], pad columns 0
  for (int i = tid * 8; i < TB * PX; i += NT * 8) {
    const int row = i / PX, col0 = i % PX;
    const float mR = sMax[row], ivR = sInv[row];
    const float* lrow = logits + row * LDL;
    struct __attribute__((aligned(16))) V8 { T x[8]; } v;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int col = col0 + q;
      float pv;
      if constexpr (RV)  // the row already holds s unless selLogits
        pv = (col < E) ? (rp.selLogits ? __expf(lrow[col] - mR) * ivR
                                       : lrow[col])
                       : 0.0f;
      else
        pv = (col < E) ? __expf(lrow[col] - mR) * ivR : 0.0f;
      fromF(pv, v.x[q]);
    }
    *reinterpret_cast<V8*>(gate_out + (size_t)(m0 + row) * PX + col0) = v;
  }

  if (!lastOfTile) {  // everyone but the tile's last arriver is done
    FM_AUX_STAMP(0, 1);
    return;
  }

  // ---- last arriver: place the tile's 128 x K selections -------------
  // sel / mCw were produced in THIS launch by other CUs: agent-scope
  // loads only (never a path the compiler may turn into a scalar-cache
  // load - see gemm_job_body's eC comment)
  const int t0 = tile * 128;
  for (int i = tid; i < 128 * K; i += NT)
    sSel[i] = __hip_atomic_load(gateSel + (size_t)t0 * K + i, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
  for (int i = tid; i < 128; i += NT)
    sCw[i] = __hip_atomic_load(gateCw + t0 + i, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  {
    // a token's K selections are distinct experts, so an entry's index
    // within the tile is the number of EARLIER tokens that selected the
    // same expert: ballot + prefix popcount per 64-token half
    const int half = wave & 1;
    const int tok = half * 64 + lane;
    uint16_t s[K];
#pragma unroll
    for (int j = 0; j < K; ++j) s[j] = sSel[tok * K + j];
    for (int e = wave >> 1; e < E; e += NWV / 2) {
      int hj = -1;
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (s[j] == (uint16_t)e) hj = j;
      const unsigned long long mk = __ballot(hj >= 0);
      const uint32_t pre = __builtin_amdgcn_mbcnt_hi(
          (uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
      if (hj >= 0) sLoc[tok * K + hj] = (uint16_t)pre;
      if (lane == 0) cntH[half * 64 + e] = (uint32_t)__popcll(mk);
    }
  }
  __syncthreads();
  if (tid < E)
    base[tid] = __hip_atomic_fetch_add(eCacc + tid, cntH[tid] + cntH[64 + tid],
                                       __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
  // ---- second ticket, taken as soon as this tile's counts are in eCacc
  // (tokenIds / kept below have no reader inside this launch); the block
  // completing it publishes the raw counts and re-zeroes the scratch
  const uint32_t nTiles = gridDim.x / SUB;
  if (gate_arrive(tilesDone, nTiles - 1, &sFlag[1]) == nTiles - 1) {
    if (tid < E) {
      eC[tid] = __hip_atomic_load(eCacc + tid, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);  // raw counts
      __hip_atomic_store(eCacc + tid, 0u, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid == 0)
      __hip_atomic_store(tilesDone, 0u, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid == 0)
    __hip_atomic_store(tileArrive + tile, 0u, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  for (int i = tid; i < 128 * K; i += NT) {
    const int tok = i / K, j = i % K;
    const int e = sSel[i];
    bool keep = false;
    if (e < E) {  // e == E only when the token's logits are all NaN/-inf
      const uint32_t slot =
          base[e] + sLoc[i] + (tok >= 64 ? cntH[e] : 0u);
      keep = slot < (uint32_t)EC;
      if (keep)
        tokenIds[(size_t)e * pEC + slot] =
            TPS{(uint32_t)(t0 + tok) | ((uint32_t)j << 28), sCw[tok]};
    }
    if (kept) kept[(size_t)(t0 + tok) * K + j] = keep ? 1 : 0;
  }
  FM_AUX_STAMP(0, 1);
}

// ---------------------------------------------------------------------------
// MX-fp8 activation quantization (dtype 5, the cfg5 regime: "CDNA4 fp8
// MFMA + token-scaling"): bf16 rows -> fp8 e4m3 bytes + per-64-element
// E8M0 block scales. Block size 64 matches the EMPIRICAL scale
// granularity of v_mfma_scale_f32_16x16x128_f8f6f4 on gfx950 (probe
// test_mx_mfma_layout_probe: the scale byte of lane-group g applies to
// the interleaved chunk pair {k: k>>6 == g&1, (k>>4)&1 == g>>1}, so a
// per-contiguous-64 scale supplied to lane-groups {0,2} (block 0) and
// {1,3} (block 1) scales every hardware block uniformly; opsel selects
// the byte). Scale = 2^e with e chosen so blockmax/2^e <= 448 (e4m3
// max); rounding RNE via v_cvt_pk_fp8_f32.
// ---------------------------------------------------------------------------

__device__ __forceinline__ uint32_t cvt2_fp8(float a, float b) {
  // pack two fp32 -> two e4m3 bytes (RNE), low half of a dword
  f32x2n v;
  v.x = a;
  v.y = b;
  return __builtin_amdgcn_cvt_pk_fp8_f32(v.x, v.y, 0u, false);
}

template <typename T>
__global__ void k_quant_mx(const T* __restrict__ in, uint8_t* __restrict__ out,
                           uint8_t* __restrict__ scales, long long nRows,
                           int K) {
  // one wave per 64-element block: lane l holds in[row][b*64 + l] ...
  // simpler: each thread walks one block serially is too slow; use
  // 64 lanes x 1 element? Layout: block j of row r -> 64 values.
  // Grid-stride over blocks; blockDim 256 = 4 waves, each wave one
  // 64-block per iteration (lane = element).
  const int wave = (int)(threadIdx.x >> 6);
  const int lane = (int)(threadIdx.x & 63);
  const long long nBlk = nRows * (K / 64);
  for (long long b = (long long)blockIdx.x * 4 + wave; b < nBlk;
       b += (long long)gridDim.x * 4) {
    const long long row = b / (K / 64);
    const int j = (int)(b % (K / 64));
    const float v = toF(in[row * K + j * 64 + lane]);
    // wave max |v|
    float m = fabsf(v);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      m = fmaxf(m, __shfl_xor(m, off, 64));
    // E8M0 exponent e: smallest power of two with blockmax/2^e <= 448
    int e = 0;
    if (m > 0.0f) {
      int ex;
      (void)frexpf(m / 448.0f, &ex);  // m/448 = f * 2^ex, f in [0.5, 1)
      e = ex;                          // 2^ex >= m/448 > 2^(ex-1)
      if (e < -126) e = -126;
      if (e > 127) e = 127;
    }
    const float inv = exp2f((float)-e);
    const uint32_t pk = cvt2_fp8(v * inv, 0.0f);
    out[row * K + j * 64 + lane] = (uint8_t)(pk & 0xFF);
    if (lane == 0) scales[row * (K / 64) + j] = (uint8_t)(127 + e);
  }
}

// ---------------------------------------------------------------------------
// Grouped expert GEMM (reference: os/processor/processor.cuh fGET preGEMM
// :339-468 / postGEMM :711-751, gemm.cuh FAA epilogue, combine :44-205).
// PHASE 0 (up):   A = x rows gathered via tokenIds[e]; B = Wup[e] [P,H];
//                 epilogue act(acc + b_up) -> xM[e]
// PHASE 1 (down): A = xM[e]; B = Wdn[e] viewed [H,P] (reference
//                 reinterpretation, moe.cuh:114-116); epilogue
//                 z = acc + b_dn; k>1: atomicAdd(O32, gate_out*z/probSum)
//                 (processor.cuh:126-168); k==1: unscaled store to moe_out
//                 (processor.cuh:173-204)
// PHASE 2 (down-direct, EP path): like 1 but plain store to out_rows[m].
// PHASE 3 (gate logits): A = x (identity rows), B = gate_w viewed [E,H]
//                 (reference quirk, moe.cuh:107-109); epilogue: plain f32
//                 store to out[m*N + col] - feeds k_gate_route. MFMA
//                 replaces the VALU logits kernel (it was ~80 us at the
//                 E=64/H=1024 8-GPU shape).
// If tokenIds == nullptr the row gather is identity and routed = n_rows
// (packed-rows mode for fm_expert_ffn).
// ---------------------------------------------------------------------------

struct GemmArgs {
  const void* A;        // phase0: x [S,H]; phase1/2: xM_e rows [pEC,K]
  const void* B;        // weight rows [N,K] (K contiguous)
  const void* bias;     // [N] or null
  void* out;            // phase0: xM_e [pEC,P]; phase2: out_rows
  float* O32;           // phase1 k>1
  void* moe_out;        // phase1 k==1
  const void* gate_out; // [S,PX]
  const TPS* tokenIds;  // [E,pEC] (this expert's row = tokenIds + e*pEC)
  const uint32_t* eC;
  long long strideAExpert;  // elements between experts in A (phase1: pEC*K)
  long long strideBExpert;  // elements between experts in B (wMats*P*H)
  long long strideOExpert;  // elements between experts in out
  int K;                // reduction dim
  int N;                // output dim
  int EC, pEC, PX;
  int topk;
  int act;
  int expertOffset;     // global expert id of blockIdx.z==0
  int nRows;            // packed-rows mode row count
  int H;                // row stride of x / O32 / moe_out
  int splitK;           // K-split factor (PHASE 1 multi only: the fp32
                        // atomicAdd combine makes split-K partials free)
  const int32_t* segExpert;  // optional [gridZ] device map: z -> weight
                             // expert (padded-EP segments; null = identity)
  int noRemap;               // debug: 1 disables the XCD block remap
  int totalJobs;             // persistent grid: total (m,n,e) tiles to
                             // cover (0 = one tile per block, classic)
  int jobsMT, jobsNT;        // tile grid dims when persistent
  int atomicLogits;          // PHASE 3: atomicAdd into fp32 out (K-split
                             // partial accumulate; fused gate)
  int slotAlways;            // PHASE 1: write the per-(token,j) combine
                             // slot even at topk==1 (scale 1; the fused
                             // kernel always reduces via k_cast_combine
                             // semantics so dropped tokens zero out)
  int sc1Out;                // epilogue stores agent-scope write-through
                             // (Guideline 16 R1 publish-large): in-launch
                             // consumers on other CUs see them after a
                             // vmcnt drain + job-count arrival, with no
                             // per-block release fence
  const void* aScales;       // MX path (dtype 5): per-64-element E8M0
                             // block scales of the quantized A operand,
                             // laid out like A with K/64 bytes per row
  void* out8;                // MX PHASE 0 (BN=256 geometry): quantize the
  void* outScales;           // activation tile in-register in the
                             // epilogue (bf16-round -> 16-lane blockmax
                             // -> e4m3) and store fp8 + E8M0 scales
                             // directly - skips the k_quant_mx pass and
                             // the bf16 xM round-trip entirely
  long long gluOffset;       // gated PHASE 0 (hidden_act 2/3): elements from
                             // an expert's Wup (slot 0, at B) to its gating
                             // projection Wglu (slot 2); N is then the
                             // EFFECTIVE width 2P and the output pitch N/2
  int nShared;               // PHASE 1, shared experts (num_shared_experts):
  int nRoutedE;              // the combine slot pitch is topk + nShared, and
                             // a z-slice e >= nRoutedE is a shared-expert
                             // slice: scale 1, no gate_out read. Both are
                             // wave-uniform; 0 / unused without shared experts
  const float* wScale;       // fp8 weights (dtype 4/5): per-output-channel
  long long wScaleStride;    // fp32 scales of B's rows (fm_set_weight_scales)
  int wScaleGlu;             // or null = 1.0. Indexed like the bias slabs:
                             // wScale + we * wScaleStride is the [N] vector of
                             // this phase's matrix (the host passes the
                             // phase's base inside the per-expert record);
                             // wScaleGlu is the distance from there to the
                             // gating projection's vector (gated PHASE 0)
};

// Per-output-channel weight scale: W_eff[n, :] = s[n] *
// W_fp8[n, :] factors out of the K sum, so the fp8-weight kernels multiply the
// fp32 accumulator by s[n] in the epilogue, ahead of bias and activation. The
// kernels test the pointer at run time; without scales the factor is 1.0f
// and acc * 1.0f is acc, bit for bit.
__device__ __forceinline__ float wscale_at(const float* sp, int col, int n) {
  return (sp && col < n) ? sp[col] : 1.0f;
}

// Gated experts (hidden_act 2 SwiGLU, 3 GeGLU): h = act(g) * u with
// g = x.Wglu^T, u = x.Wup^T, both still fp32 accumulators. The up GEMM
// runs over an effective N = 2P whose tile-local B rows are sourced
// INTERLEAVED from the two projections (16-row fragments in the MFMA
// kernels, single rows in the fp32 kernel), so g and u of one output
// element always sit in the same thread.
__device__ __forceinline__ float gate_act(float v, int act) {
  return act == 2 ? v / (1.0f + expf(-v))
                  : 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
}

// address-space helpers for global_load_lds (direct HBM->LDS DMA)
typedef __attribute__((address_space(1))) const uint32_t gas_u32;
typedef __attribute__((address_space(3))) uint32_t las_u32;

template <typename ET, int PHASE, int ACT, bool HAS_BIAS, typename WET = ET,
          bool TAILA = false>
__global__ __launch_bounds__(256) void k_group_gemm_bf16(GemmArgs a) {
  using vec8 = typename ETr<ET>::vec8;
  constexpr int BM = 128, BN = 128, BK = 64;
  constexpr bool GATED = (PHASE == 0) && (ACT >= 2);
  // WET is the WEIGHT (B operand) storage element: == ET normally, or
  // fp8e4m3 for the config-5 fp8-weight path (W8A16: B staged through
  // glds as raw fp8 bytes, dequantized to bf16 at fragment-read time so
  // the MFMA stream and the all-glds staging pipeline are unchanged and
  // B's HBM/LDS traffic halves).
  constexpr int BEZ = (int)sizeof(WET);
  constexpr int BCH = BK * BEZ / 16;  // 16B chunks per B row (8 or 4)
  // ONE shared arena (a second __shared__ object would force a vmcnt(0)
  // drain before every ds_read beside glds - guide par.5 trap 4a).
  // A/B tiles are LINEAR [128][64] bf16 (glds writes lane-linearly); the
  // bank swizzle lives on the SOURCE chunk index and the fragment-read
  // address (rule 21): chunk' = chunk ^ (row & 7) (bf16 B); for fp8 B
  // (64B rows) it is chunk16' = chunk16 ^ ((row >> 2) & 3), which makes
  // the b64 fragment reads bank-conflict-free.
  __shared__ __attribute__((aligned(16))) char smem[
      BM * BK * 2 + BN * BK * BEZ + BM * 8 + 16];
  ET* Alds = reinterpret_cast<ET*>(smem);
  WET* Blds = reinterpret_cast<WET*>(smem + BM * BK * 2);
  TPS* sTps = reinterpret_cast<TPS*>(smem + BM * BK * 2 + BN * BK * BEZ);
  uint32_t* sRouted = reinterpret_cast<uint32_t*>(sTps + BM);

  const int skS = a.splitK > 0 ? a.splitK : 1;
  const int e = blockIdx.z % (gridDim.z / skS);
  const int ksplitS = blockIdx.z / (gridDim.z / skS);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int K = a.K, N = a.N;
  const int kLenS = K / skS;
  const int kStartS = ksplitS * kLenS;

  const int we = a.segExpert ? a.segExpert[e] : e;  // weight/bias expert
  if constexpr (PHASE == 3) {
    // gate-logits phase: block (0,0,0) zeroes eC for the route kernel
    // that follows (saves a launch-bound memset per forward); EC field
    // carries the expert count here
    if (a.eC && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
      uint32_t* ec = const_cast<uint32_t*>(a.eC);
      for (int i = tid; i < a.EC; i += 256) ec[i] = 0;
    }
  }
  const TPS* tpsE = a.tokenIds ? a.tokenIds + (size_t)e * a.pEC : nullptr;
  if (tid == 0) {
    *sRouted = tpsE ? min(a.eC[e], (uint32_t)a.EC) : (uint32_t)a.nRows;
  }
  __syncthreads();
  const uint32_t routed = *sRouted;
  if ((uint32_t)m0 >= routed) return;  // empty tile (0-token expert / tail)

  if (tid < BM) {
    TPS t{0u, 1.0f};
    if ((uint32_t)(m0 + tid) < routed) {
      t = tpsE ? tpsE[m0 + tid] : TPS{(uint32_t)(m0 + tid), 1.0f};
    }
    sTps[tid] = t;
  }
  __syncthreads();

  const ET* __restrict__ Ag = reinterpret_cast<const ET*>(a.A);
  const WET* __restrict__ Bg =
      reinterpret_cast<const WET*>(a.B) + (size_t)we * a.strideBExpert;

  // accumulators: wave (wr,wc) owns the 64x64 subtile at (wr*64, wc*64)
  const int wr = wave >> 1, wc = wave & 1;
  f32x4 accv[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) accv[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // glds staging: 16 KiB per tile = 16 wave-instructions of 1 KiB; wave w
  // issues groups w*4..w*4+3; lane l covers row grp*8 + l/8, chunk l%8.
  // Source chunk is XOR-swizzled: sc = (l%8) ^ (l/8) (row&7 == l/8).
  const int grow8 = lane >> 3;           // row within the 8-row group
  const int schunk = (lane & 7) ^ grow8;  // swizzled 16B chunk index
  // B staging geometry in WET units: 1KiB glds group covers 1024/(BK*BEZ)
  // rows; lane -> (row-in-group, chunk) with the WET-specific swizzle.
  constexpr int BGW = BN * BK * BEZ / 1024 / 4;  // B groups per wave (4 or 2)
  const int bgrow = lane / BCH;
  const int bsc = (lane % BCH) ^ (BEZ == 1 ? ((bgrow >> 2) & 3) : bgrow);
  const int aRowStride = (PHASE == 0) ? a.H : K;
  const size_t aBase = (size_t)e * a.strideAExpert;  // 0 for the x-gather up phase
  for (int kt = kStartS; kt < kStartS + kLenS; kt += BK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int grp = wave * 4 + i;
      const int row = grp * 8 + grow8;
      size_t arow = (PHASE == 0) ? (size_t)tpsTok(sTps[row].tokenIdx)
                                 : (size_t)(m0 + row);
      // TAILA: the logits GEMM of a decode-sized forward reads the
      // caller's x, which ends at row nRows < BM
      if constexpr (TAILA) arow = min(arow, (size_t)routed - 1);
      const ET* asrc = Ag + aBase + arow * aRowStride + kt + schunk * 8;
      __builtin_amdgcn_global_load_lds(
          (gas_u32*)asrc, (las_u32*)(Alds + grp * 512), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < BGW; ++i) {
      const int grp = wave * BGW + i;
      const int row = grp * (1024 / (BK * BEZ)) + bgrow;
      int brow = min(n0 + row, N - 1);
      const WET* bexp = Bg;
      if constexpr (GATED) {
        // fragment-interleaved source: even 16-row fragments read Wglu,
        // odd ones Wup, same P rows; clamp per half (N is 2P here)
        const int f = row >> 4;
        brow = min((n0 >> 1) + (f >> 1) * 16 + (row & 15), (N >> 1) - 1);
        if ((f & 1) == 0) bexp += a.gluOffset;
      }
      const WET* bsrc = bexp + (size_t)brow * K + kt + bsc * (16 / BEZ);
      __builtin_amdgcn_global_load_lds(
          (gas_u32*)bsrc, (las_u32*)((char*)Blds + grp * 1024), 16, 0, 0);
    }
    __syncthreads();  // carries the vmcnt(0) glds drain (guide par.5)
#pragma unroll
    for (int s = 0; s < 2; ++s) {  // two K=32 MFMA steps per tile
      vec8 af[4], bf[4];
      const int rl = lane & 15;
      const int cbase = 4 * s + (lane >> 4);  // 16B chunk before swizzle
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int R = wr * 64 + mi * 16 + rl;
        af[mi] = *reinterpret_cast<const vec8*>(
            &Alds[R * BK + ((cbase ^ (R & 7)) * 8)]);
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int R = wc * 64 + ni * 16 + rl;
        if constexpr (BEZ == 1) {
          // fp8 B: 8-byte read (the (R>>2)&3 chunk16 swizzle makes the 16
          // lanes of each quarter-wave hit 16 distinct banks), dequant to
          // bf16 in regs before the MFMA
          const int c16 = (cbase >> 1) ^ ((R >> 2) & 3);
          const uint32_t* bp = reinterpret_cast<const uint32_t*>(
              (const char*)Blds + (size_t)R * BK + c16 * 16 + (cbase & 1) * 8);
          bf[ni] = dequant_fp8x8_bf16(bp[0], bp[1]);
        } else {
          bf[ni] = *reinterpret_cast<const vec8*>(
              &Blds[R * BK + ((cbase ^ (R & 7)) * 8)]);
        }
      }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          accv[mi][ni] = ETr<ET>::mfma(af[mi], bf[ni], accv[mi][ni]);
    }
    __syncthreads();
  }

  // epilogue: C/D map for 16x16 MFMA: col = lane&15, row = (lane>>4)*4 + r.
  // Bias and combine scales are HOISTED (a per-element bias load made
  // hipcc emit one dependent global_load+vmcnt(0) per output - guide
  // par.5 trap 4c, profiles/r01); activation is a compile-time template.
  const int cl = lane & 15;
  const int r0 = (lane >> 4) * 4;
  float* sScale = reinterpret_cast<float*>(Alds);  // reuse; loop is done
  // multi: write the per-(token, j) combine slot. A shared-expert slice
  // (e >= nRoutedE) is unscaled and reads no gate_out column.
  const bool multi = (PHASE == 1) && (a.topk > 1 || a.slotAlways);
  const bool scaled =
      (PHASE == 1) && a.topk > 1 && !(a.nShared && e >= a.nRoutedE);
  const int nSlot = a.topk + a.nShared;
  if constexpr (PHASE == 1) {
    if (scaled) {
      __syncthreads();
      if (tid < BM) {
        const TPS tp = sTps[tid];
        float sc = 0.0f;
        if ((uint32_t)(m0 + tid) < routed)
          sc = toF(reinterpret_cast<const ET*>(
                   a.gate_out)[(size_t)tpsTok(tp.tokenIdx) * a.PX +
                               a.expertOffset + e]) / tp.probSum;
        sScale[tid] = sc;
      }
      __syncthreads();
    }
  }
  float bv[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (HAS_BIAS) {
    // multi-expert launches (strideBExpert > 0) carry per-expert bias
    // slabs [nLx, N]; the packed-rows single-expert API passes the
    // expert's own slab (stride 0)
    const ET* bptr = reinterpret_cast<const ET*>(a.bias) +
                     (a.strideBExpert ? (size_t)we * N : 0);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int col = n0 + wc * 64 + ni * 16 + cl;
      if (col < N) bv[ni] = toF(bptr[col]);
    }
  }
  // fp8 weights: this job's per-column weight scales, loaded once beside bv
  // (gated: sv[2j] is s_glu and sv[2j+1] is s_up of the same P column)
  constexpr bool WS = (BEZ == 1) && (PHASE != 3);
  float sv[4] = {1.f, 1.f, 1.f, 1.f};
  if constexpr (WS) {
    const float* sp =
        a.wScale ? a.wScale + (size_t)we * a.wScaleStride : nullptr;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      if constexpr (GATED) {
        const int col = (n0 >> 1) + wc * 32 + (ni >> 1) * 16 + cl;
        sv[ni] = wscale_at(sp ? sp + ((ni & 1) ? 0 : a.wScaleGlu) : nullptr,
                           col, N >> 1);
      } else {
        sv[ni] = wscale_at(sp, n0 + wc * 64 + ni * 16 + cl, N);
      }
    }
  }
  // accumulator element (mi, ni, r) with its weight scale applied
  auto accS = [&](int mi, int ni, int r) __attribute__((always_inline)) {
    if constexpr (WS) return accv[mi][ni][r] * sv[ni];
    else return accv[mi][ni][r];
  };
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wr * 64 + mi * 16 + r0 + r;
      const int m = m0 + row;
      if ((uint32_t)m >= routed) continue;
      const TPS tp = sTps[row];
      const float rowScale = scaled ? sScale[row] : 1.0f;
      if constexpr (GATED) {
        // fragment pairs (2j, 2j+1) hold (g, u) of the same (row, p)
        const int P = N >> 1;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int col = (n0 >> 1) + wc * 32 + j * 16 + cl;
          if (col >= P) continue;
          reinterpret_cast<ET*>(a.out)[(size_t)e * a.strideOExpert +
                                       (size_t)m * P + col] =
              ETr<ET>::fromf(gate_act(accS(mi, 2 * j, r), ACT) *
                             accS(mi, 2 * j + 1, r));
        }
        continue;
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int col = n0 + wc * 64 + ni * 16 + cl;
        if (col >= N) continue;
        float v = accS(mi, ni, r) + bv[ni];
        if constexpr (PHASE == 0) {
          v = (ACT == 0) ? fmaxf(v, 0.0f)
                         : 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
          reinterpret_cast<ET*>(a.out)[(size_t)e * a.strideOExpert +
                                         (size_t)m * N + col] =
              ETr<ET>::fromf(v);
        } else if constexpr (PHASE == 1) {
          if (multi) {
            // non-atomic per-(token, j) combine slot (summed with the
            // kept mask in k_cast_combine; replaces fp32 atomics)
            reinterpret_cast<ET*>(a.O32)[
                ((size_t)tpsTok(tp.tokenIdx) * nSlot + tpsJ(tp.tokenIdx)) *
                    a.H + col] = ETr<ET>::fromf(v * rowScale);
          } else {
            reinterpret_cast<ET*>(
                a.moe_out)[(size_t)tpsTok(tp.tokenIdx) * a.H + col] =
                ETr<ET>::fromf(v);
          }
        } else if constexpr (PHASE == 2) {  // packed-rows direct output
          reinterpret_cast<ET*>(a.out)[(size_t)e * a.strideOExpert +
                                       (size_t)m * N + col] =
              ETr<ET>::fromf(v);
        } else {  // PHASE 3: gate logits, fp32 (atomic when K-split)
          if (skS > 1)
            atomicAdd(&reinterpret_cast<float*>(a.out)[(size_t)m * N + col], v);
          else
            reinterpret_cast<float*>(a.out)[(size_t)m * N + col] = v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Big-tile grouped GEMM, bf16 MFMA: 256xBN (BN 256 or 128), BK=64,
// 512 threads = 8 waves (2M x 4N), per-wave 128 x BN/4 as 8 x BN/64
// mfma_f32_16x16x32_bf16 fragments. Double-buffered glds staging with
// COUNTED vmcnt + raw s_barrier (the guide's deep-pipeline recipe: a
// __syncthreads here would drain vmcnt(0) and expose full HBM latency
// every K-tile - measured 47% wave-park, profiles/r01 PMC). Used for the
// large-M expert shapes; the 128^2 kernel remains for small tiles.
// Same phase semantics/epilogues as k_group_gemm_bf16.
// ---------------------------------------------------------------------------

// -DFM_GEMM_STAMPS (measurement build only, tools/gemm_phase_stamps.py):
// thread 0 of each block records the constant 100 MHz wall clock at job
// entry, first MFMA, end of K-loop and end of epilogue of every big-tile
// job and writes the four stamps to g_gemmStamps[PHASE][block][job].
// The default build contains none of this.
#ifdef FM_GEMM_STAMPS
constexpr int FM_STAMP_PHASES = 4, FM_STAMP_BLOCKS = 512, FM_STAMP_JOBS = 4;
__device__ unsigned long long
    g_gemmStamps[FM_STAMP_PHASES][FM_STAMP_BLOCKS][FM_STAMP_JOBS][4];
#define FM_STAMP(i)                                                           \
  do {                                                                        \
    if (threadIdx.x == 0) fmStamp[i] = __builtin_amdgcn_s_memrealtime();      \
  } while (0)
#else
#define FM_STAMP(i) do {} while (0)
#endif

// effective staging depth for a (BM, BN, WET, STAGES) tile: degrade
// triple buffering to double when it would not fit the 160 KB LDS
// per-row epilogue metadata behind the stage buffers: two copies (job
// parity) of sTps[BM] (8 B) and sScale[BM] (4 B), plus a 16-B pad
__host__ __device__ constexpr int gemm_meta_bytes(int BM) {
  return 2 * BM * 8 + 2 * BM * 4 + 16;
}

template <int BM, int BN, int BEZ, int STAGES>
constexpr int gemm_se() {
  return (STAGES == 3 && 3 * BM * 64 * 2 + 3 * BN * 64 * BEZ +
                                 gemm_meta_bytes(BM) > 160 * 1024)
             ? 2 : STAGES;
}

// LDS arena bytes the tile body needs (mirrored on the host when sizing
// the fused kernel's dynamic arena)
template <int BM, int BN, int BEZ, int STAGES>
constexpr int gemm_lds_bytes() {
  constexpr int SE = gemm_se<BM, BN, BEZ, STAGES>();
  return SE * BM * 64 * 2 + SE * BN * 64 * BEZ + gemm_meta_bytes(BM);
}

// compile-time bool handed to the epilogue's generic lambda
template <bool B> struct BoolC { static constexpr bool value = B; };

// Four consecutive output columns of one row (col0 .. col0+3, nValid of
// them inside N) from one lane. Wide path: packed conversion + ONE 8-byte
// store (16-byte for fp32). SC1 keeps the agent-scope write-through of
// storeElem on the wide word (relaxed atomic store at agent scope ->
// global_store_dwordx2 ... sc1). A group that straddles N, or a row base
// that is not wide-aligned (vecOK false), falls back to element stores.
template <bool SC1, typename ET>
__device__ __forceinline__ void storeRow4(ET* p, const float (&v)[4],
                                          int nValid, bool vecOK) {
  if (vecOK && nValid >= 4) {
    const uint64_t w = (uint64_t)ETr<ET>::pack2(v[0], v[1]) |
                       ((uint64_t)ETr<ET>::pack2(v[2], v[3]) << 32);
    if constexpr (SC1)
      __hip_atomic_store(reinterpret_cast<uint64_t*>(p), w, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    else
      *reinterpret_cast<uint64_t*>(p) = w;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < nValid) storeElem(p + r, ETr<ET>::fromf(v[r]), SC1);
  }
}

// Eight consecutive output columns of one row from one lane, already
// converted and packed two elements per dword (w[0] = columns 0-1 ..
// w[3] = columns 6-7), nValid of them inside N. p is 16-byte aligned.
// Wide path: ONE 16-byte store. A group that straddles N falls back to
// 8-byte halves and then to elements, storing the same packed bits.
template <typename ET>
__device__ __forceinline__ void storeRow8(ET* p, const uint32_t (&w)[4],
                                          int nValid) {
  static_assert(sizeof(ET) == 2, "packed pairs of 2-byte elements");
  if (nValid >= 8) {
    *reinterpret_cast<u32x4*>(p) = u32x4{w[0], w[1], w[2], w[3]};
  } else {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int nv = nValid - 4 * h;
      if (nv >= 4) {
        *reinterpret_cast<uint64_t*>(p + 4 * h) =
            (uint64_t)w[2 * h] | ((uint64_t)w[2 * h + 1] << 32);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (r < nv)
            reinterpret_cast<uint16_t*>(p)[4 * h + r] =
                (uint16_t)(w[2 * h + (r >> 1)] >> (16 * (r & 1)));
      }
    }
  }
}

// ---------------------------------------------------------------------------
// One (e, m0, n0, ksplit) tile job of the big-tile grouped GEMM: the
// shared body of k_group_gemm_bf16_big (classic multi-kernel path) and
// k_moe_fused (single-launch persistent path). act / hasBias are
// runtime here; the classic kernels pass template constants that fold
// after inlining. Layout/state contracts documented at the kernel below.
// ---------------------------------------------------------------------------
// RT_SC1: honour a.sc1Out (agent-scope write-through epilogue stores).
// Only the fused kernel has in-launch consumers, so only its walks
// instantiate the sc1 epilogues; the classic kernels compile them out.
template <typename ET, int PHASE, int BN, int BM, typename WET, int STAGES,
          int CK = 0, int CN = 0, bool RT_SC1 = false, bool GATED = false>
__device__ __forceinline__ bool gemm_job_body(
    const GemmArgs& a, char* smemBase, int e, int ksplit, int m0, int n0,
    int act, bool hasBias, int par, int jobLocal = 0) {
  // par: which copy of the per-row metadata (sTps/sScale) this job uses.
  // The caller flips it after every job that RAN: a job then never
  // rewrites the copy the previous job's epilogue may still be reading
  // (every wave passes a barrier of job t+1 before job t+2 starts), so
  // no barrier is needed between one job's epilogue and the next
  // job's prologue. An empty job passes no barrier and must not flip.
  using vec8 = typename ETr<ET>::vec8;
#ifdef FM_GEMM_STAMPS
  unsigned long long fmStamp[4] = {0, 0, 0, 0};
#endif
  (void)jobLocal;
  FM_STAMP(0);
  constexpr int BK = 64;
  constexpr int NF = BN / 64;           // B fragments per wave (4 or 2)
  constexpr int MI = BM / 32;           // A fragments per wave (8 or 4)
  constexpr int BEZ = (int)sizeof(WET);
  constexpr int BCH = BK * BEZ / 16;        // 16B chunks per B row
  constexpr int AGRP = BM * BK * 2 / 1024;  // glds 1KiB groups per A tile
  constexpr int BGRP = BN * BK * BEZ / 1024;
  constexpr int GPW_A = AGRP / 8, GPW_B = BGRP / 8;  // per wave
  constexpr int GPT = GPW_A + GPW_B;    // glds per wave per K-tile
  constexpr int SE = gemm_se<BM, BN, BEZ, STAGES>();
  ET* Abase = reinterpret_cast<ET*>(smemBase);      // SE x [BM][BK]
  WET* Bbase = reinterpret_cast<WET*>(smemBase + SE * BM * BK * 2);
  TPS* sTps = reinterpret_cast<TPS*>(
      smemBase + SE * BM * BK * 2 + SE * BN * BK * BEZ) + par * BM;
  float* sScale = reinterpret_cast<float*>(
      smemBase + SE * BM * BK * 2 + SE * BN * BK * BEZ + 2 * BM * 8) + par * BM;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  // CK/CN: compile-time K/N for the BASELINE shape dictionary (the
  // reference's own architecture freezes these in flashmoe_config.json
  // as compile-time constants); 0 = runtime (generic path). Constant
  // shapes fold the staging address math and fully determine the
  // K-tile trip count (the probe ladder's "template generality" gap).
  const int K = CK ? CK : a.K;
  const int N = CN ? CN : a.N;
  const int sk = a.splitK > 0 ? a.splitK : 1;
  const int kLen = K / sk;            // this split's K range
  const int kStart = ksplit * kLen;

  const TPS* tpsE = a.tokenIds ? a.tokenIds + (size_t)e * a.pEC : nullptr;
  // routed count: every wave reads it itself (no LDS round trip, no
  // barrier) and makes it wave-uniform. An agent-scope load, not a
  // scalar-cache one: in the fused kernel eC is produced earlier in the
  // SAME launch, which the scalar cache is not coherent with.
  uint32_t routed = (uint32_t)a.nRows;
  if (tpsE)
    routed = min((uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(
                     a.eC + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)),
                 (uint32_t)a.EC);
  if ((uint32_t)m0 >= routed) return false;  // empty tile (block-uniform)
  const int mCap = a.tokenIds ? a.pEC : a.nRows;  // A-row clamp bound
  const int we = a.segExpert ? a.segExpert[e] : e;  // weight/bias expert

  const ET* __restrict__ Ag = reinterpret_cast<const ET*>(a.A);
  const WET* __restrict__ Bg =
      reinterpret_cast<const WET*>(a.B) + (size_t)we * a.strideBExpert;

  // per-lane glds source bases, hoisted out of the K loop
  const int grow8 = lane >> 3;
  const int schunk = (lane & 7) ^ grow8;
  // B staging geometry in WET units: 1KiB group = 1024/(BK*BEZ) rows;
  // fp8 swizzle is on the 16B chunk16 index: ^ ((row >> 2) & 3)
  const int bgrow = lane / BCH;
  const int bsc = (lane % BCH) ^ (BEZ == 1 ? ((bgrow >> 2) & 3) : bgrow);
  const int aRowStride = K;  // == a.H (up, logits) / a.K (down) by layout
  const size_t aBase = (size_t)e * a.strideAExpert;  // 0 for the x-gather up phase
  const ET* aSrc[GPW_A];
  const WET* bSrc[GPW_B];
  // The staging lanes load the routing entries of their own A rows
  // straight from global (8 lanes share a row): no LDS round trip sits
  // between tokenIds and the first A stage. Issued FIRST, so the B half
  // of stage 0 below overlaps their latency.
  TPS tpsv[GPW_A];
#pragma unroll
  for (int i = 0; i < GPW_A; ++i) {
    const int row = (wave * GPW_A + i) * 8 + grow8;
    TPS t{0u, 1.0f};
    if ((uint32_t)(m0 + row) < routed)
      t = tpsE ? tpsE[m0 + row] : TPS{(uint32_t)(m0 + row), 1.0f};
    tpsv[i] = t;
  }
#pragma unroll
  for (int i = 0; i < GPW_B; ++i) {
    const int row = (wave * GPW_B + i) * (1024 / (BK * BEZ)) + bgrow;
    if constexpr (GATED) {
      // Fragment-interleaved source (N is the effective 2P): tile-local
      // row R lies in 16-row fragment f = R / 16; even f reads Wglu, odd f
      // reads Wup, both at P row n0/2 + (f/2)*16 + R%16, clamped per half.
      // A 1 KiB group covers 8 or 16 rows, so it never straddles a
      // fragment. A wave's fragments start at an even f (NF is even), so
      // accv[mi][2j] / accv[mi][2j+1] are g / u of the same (row, p).
      static_assert(PHASE == 0, "gated epilogue is the up phase only");
      const int f = row >> 4;
      const int prow =
          min((n0 >> 1) + (f >> 1) * 16 + (row & 15), (N >> 1) - 1);
      bSrc[i] = Bg + ((f & 1) ? 0 : a.gluOffset) + (size_t)prow * K + kStart +
                bsc * (16 / BEZ);
    } else {
      bSrc[i] =
          Bg + (size_t)min(n0 + row, N - 1) * K + kStart + bsc * (16 / BEZ);
    }
  }

  auto stageA = [&](int kt, int buf) {
#pragma unroll
    for (int i = 0; i < GPW_A; ++i)
      __builtin_amdgcn_global_load_lds(
          (gas_u32*)(aSrc[i] + kt),
          (las_u32*)(Abase + buf * BM * BK + (wave * GPW_A + i) * 512), 16, 0, 0);
  };
  auto stageB = [&](int kt, int buf) {
#pragma unroll
    for (int i = 0; i < GPW_B; ++i)
      __builtin_amdgcn_global_load_lds(
          (gas_u32*)(bSrc[i] + kt),
          (las_u32*)((char*)Bbase + buf * BN * BK * BEZ +
                     (wave * GPW_B + i) * 1024), 16, 0, 0);
  };
  auto stage = [&](int kt, int buf) {
    stageA(kt, buf);
    stageB(kt, buf);
  };

  // prologue: the B half of stage 0 (weights depend on nothing) goes out
  // before the A source rows are known
  stageB(0, 0);
#pragma unroll
  for (int i = 0; i < GPW_A; ++i) {
    const int row = (wave * GPW_A + i) * 8 + grow8;
    const size_t arow = (PHASE == 0) ? (size_t)tpsTok(tpsv[i].tokenIdx)
                                     : (size_t)min(m0 + row, mCap - 1);
    aSrc[i] = Ag + aBase + arow * aRowStride + kStart + schunk * 8;
  }
  stageA(0, 0);
  // slot: write the per-(token, j) combine slot; scaled only at k>1
  // (the reference's k==1 CombineMode::single semantics are unscaled,
  // processor.cuh:173-204)
  // A shared-expert slice (e >= nRoutedE, num_shared_experts > 0) is
  // unscaled and reads no gate_out column; the slot pitch counts the
  // shared slots. Both are block-uniform scalars.
  const bool slot = (PHASE == 1) && (a.topk > 1 || a.slotAlways);
  const bool scaled =
      (PHASE == 1) && a.topk > 1 && !(a.nShared && e >= a.nRoutedE);
  const int nSlot = a.topk + a.nShared;
  // PHASE 1 row scale (gate prob / probSum): fetched here, once per row,
  // so it is in LDS long before the epilogue and needs no barrier of its
  // own. Issued BEFORE the second prologue stage: the counted vmcnt
  // below then still leaves exactly that stage's GPT loads outstanding.
  const bool metaLane = (lane & 7) == 0;  // one lane per A row
  ET gateRaw[GPW_A];
  if constexpr (PHASE == 1) {
#pragma unroll
    for (int i = 0; i < GPW_A; ++i) {
      const int row = (wave * GPW_A + i) * 8 + grow8;
      gateRaw[i] = ETr<ET>::fromf(0.0f);
      if (scaled && metaLane && (uint32_t)(m0 + row) < routed)
        gateRaw[i] = reinterpret_cast<const ET*>(
            a.gate_out)[(size_t)tpsTok(tpsv[i].tokenIdx) * a.PX +
                        a.expertOffset + e];
    }
  }

  const int wr = wave >> 2, wc = wave & 3;  // 2M x 4N wave grid
  f32x4 accv[MI][NF];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) accv[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // one-barrier 2-phase schedule (guide T3 minimum recipe): stage tile
  // t+1 into the other buffer FIRST, compute tile t, then ONE
  // vmcnt(0)+barrier per tile (the drain is cheap: the stage had the
  // whole compute phase to land).
  const int nK = kLen / BK;
  // (stage 0 was issued in the prologue above, B half first)
  if constexpr (SE == 3) {
    if (nK > 1) {
      stage(BK, 1);
      wait_vmcnt<GPT>();  // tile 0 landed; tile 1 still in flight
    } else {
      wait_vmcnt<0>();
    }
  } else {
    wait_vmcnt<0>();
  }
  // per-row epilogue metadata into this job's copy; the barrier below
  // (the first one every wave passes) publishes it
  if (metaLane) {
#pragma unroll
    for (int i = 0; i < GPW_A; ++i) {
      const int row = (wave * GPW_A + i) * 8 + grow8;
      sTps[row] = tpsv[i];
      if constexpr (PHASE == 1)
        sScale[row] = toF(gateRaw[i]) / tpsv[i].probSum;
    }
  }
  // raw barrier (a __syncthreads would drain the in-flight tile 1):
  // the metadata ds_writes are the only LDS ops outstanding
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  FM_STAMP(1);
  for (int t = 0; t < nK; ++t) {
    // STAGES==2: staggered staging - waves 0-3 stage tile t+1 before
    // their first MFMA half, waves 4-7 between the halves, so on each
    // SIMD the paired waves run complementary {stage issue | MFMA}
    // segments instead of lockstep (microarch guide, two-waves-per-SIMD).
    // STAGES==3: stage t+2 up front; the latency budget is two compute
    // phases, so no stagger is needed.
    const int pre = t + SE - 1;  // tile staged this iteration
    const bool stageNow = pre < nK;
    // stagger only pays on the wide (NF==4) stream; the BN=128 kernel's
    // shorter MFMA halves lose more to the mid-stream insertion (measured)
    const bool late = (SE == 2) && (NF == 4) && wave >= 4;
    if (stageNow && !late) stage(pre * BK, pre % SE);
    const ET* Al = Abase + (t % SE) * BM * BK;
    const WET* Bl = Bbase + (t % SE) * BN * BK;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (s == 1 && late && stageNow) {
        __builtin_amdgcn_s_setprio(0);
        stage(pre * BK, pre % SE);
        __builtin_amdgcn_s_setprio(1);
      }
      vec8 af[MI], bfr[NF];
      const int rl = lane & 15;
      const int cbase = 4 * s + (lane >> 4);
      auto aread = [&](int mi) {
        const int R = wr * (BM / 2) + mi * 16 + rl;
        af[mi] = *reinterpret_cast<const vec8*>(
            &Al[R * BK + ((cbase ^ (R & 7)) * 8)]);
      };
      // Round-robin reads and MFMAs, pinned with sched_barrier(0): each
      // MFMA pair then waits (partial lgkmcnt) only on fragments read a
      // group earlier, instead of the scheduler's whole-segment
      // lgkmcnt(0) drain before the first MFMA (seen in the .s).
#pragma unroll
      for (int ni = 0; ni < NF; ++ni) {
        const int R = wc * (BN / 4) + ni * 16 + rl;
        if constexpr (BEZ == 1) {
          const int c16 = (cbase >> 1) ^ ((R >> 2) & 3);
          const uint32_t* bp = reinterpret_cast<const uint32_t*>(
              (const char*)Bl + (size_t)R * BK + c16 * 16 + (cbase & 1) * 8);
          bfr[ni] = dequant_fp8x8_bf16(bp[0], bp[1]);
        } else {
          bfr[ni] = *reinterpret_cast<const vec8*>(
              &Bl[R * BK + ((cbase ^ (R & 7)) * 8)]);
        }
      }
      aread(0);
      aread(1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int g2 = 0; g2 < MI / 2; ++g2) {
        if (g2 < MI / 2 - 1) {
          aread(2 * g2 + 2);
          aread(2 * g2 + 3);
        }
#pragma unroll
        for (int mi = 2 * g2; mi < 2 * g2 + 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < NF; ++ni)
            // operands swapped (B fragment first): the accumulator then
            // holds C^T's layout - lane & 15 is the output ROW and
            // 4 * (lane >> 4) + r are four CONSECUTIVE output columns, so
            // the epilogue stores a row's columns as one wide word. Same
            // dot products in the same K order.
            accv[mi][ni] = ETr<ET>::mfma(bfr[ni], af[mi], accv[mi][ni]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    if constexpr (SE == 3) {
      // only t+1 must have landed; t+2 (the GPT glds issued this
      // iteration) may still be in flight
      if (stageNow) wait_vmcnt<GPT>(); else wait_vmcnt<0>();
    } else {
      wait_vmcnt<0>();  // t+1 landed
    }
    __builtin_amdgcn_s_barrier();  // readers done AND next tile ready
  }

  FM_STAMP(2);
  // epilogue (same semantics as k_group_gemm_bf16). Swapped-operand
  // accumulator layout: lane & 15 is the row inside fragment mi, and
  // accv[mi][ni][0..3] are columns cq..cq+3 of fragment ni - so the row
  // predicate, the sTps/sScale lookup and the row's output address are
  // formed once per (lane, mi), and each (mi, ni) is one wide store.
  // Reads only sTps/sScale of this job's copy: the stage buffers are
  // free for the next job's prologue as soon as the K-loop ends.
  const int rl16 = lane & 15;
  const int cq = (lane >> 4) * 4;
  const int nBase = n0 + wc * (BN / 4) + cq;  // column of accv[.][0][0]
  float bv[NF][4];
#pragma unroll
  for (int ni = 0; ni < NF; ++ni)
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[ni][r] = 0.f;
  if (hasBias && ksplit == 0) {  // split partials add the bias exactly once
    // per-expert bias slabs when multi-expert (see the 128^2 kernel)
    const ET* bptr = reinterpret_cast<const ET*>(a.bias) +
                     (a.strideBExpert ? (size_t)we * N : 0);
#pragma unroll
    for (int ni = 0; ni < NF; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = nBase + ni * 16 + r;
        if (col < N) bv[ni][r] = toF(bptr[col]);
      }
  }
  // fp8 weights: this job's per-column weight scales, loaded once beside bv
  // and shaped like it (sv[ni][r] belongs to accv[.][ni][r]). Gated: fragment
  // 2j is g and 2j+1 is u of P columns pBase + j*16 + r, so the pair takes
  // s_glu and s_up of the same columns. K-split partials each take the
  // factor (it distributes over their sum).
  constexpr bool WS = (BEZ == 1) && (PHASE != 3);
  float sv[WS ? NF : 1][4];
  if constexpr (WS) {
    const float* sp =
        a.wScale ? a.wScale + (size_t)we * a.wScaleStride : nullptr;
#pragma unroll
    for (int ni = 0; ni < NF; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (GATED) {
          const int col =
              (n0 >> 1) + wc * (BN / 8) + cq + (ni >> 1) * 16 + r;
          sv[ni][r] = wscale_at(
              sp ? sp + ((ni & 1) ? 0 : a.wScaleGlu) : nullptr, col, N >> 1);
        } else {
          sv[ni][r] = wscale_at(sp, nBase + ni * 16 + r, N);
        }
      }
  }
  // accumulator element (mi, ni, r) with its weight scale applied
  auto accS = [&](int mi, int ni, int r) __attribute__((always_inline)) {
    if constexpr (WS) return accv[mi][ni][r] * sv[ni][r];
    else return accv[mi][ni][r];
  };
  // per-expert / per-tile output base, hoisted out of the element loops;
  // wide stores need every row base 8-byte (fp32: 16-byte) aligned
  using OT = typename std::conditional<PHASE == 3, float, ET>::type;
  OT* outBase;
  long long rowPitch;  // elements between consecutive output rows
  if constexpr (PHASE == 1) {
    outBase = reinterpret_cast<OT*>(slot ? a.O32 : a.moe_out);
    rowPitch = a.H;
  } else if constexpr (PHASE == 3) {
    outBase = reinterpret_cast<OT*>(a.out);
    rowPitch = N;
  } else {
    outBase = reinterpret_cast<OT*>(a.out) + (size_t)e * a.strideOExpert;
    rowPitch = GATED ? (N >> 1) : N;  // gated: xM is [pEC, P], N is 2P
  }
  const bool vecOK =
      (rowPitch & 3) == 0 &&
      (reinterpret_cast<uintptr_t>(outBase) & (4 * sizeof(OT) - 1)) == 0;
  // 16-byte stores of eight 2-byte elements: every row base 16-byte aligned
  const bool vec16OK =
      (rowPitch & 7) == 0 && (reinterpret_cast<uintptr_t>(outBase) & 15) == 0;
  // the 16-byte path exists where a (lane, mi) has a PAIR of packed
  // 2-byte outputs (the gated BN=128 tile has one and keeps 8 bytes)
  constexpr int NOUT = GATED ? NF / 2 : NF;  // packed outputs per mi
  constexpr bool W16 = PHASE != 3 && NOUT >= 2;

  // interior tile (every column group wholly inside N, rows wide-
  // aligned): no column predicate at all. Ragged tiles take the checked
  // instantiation.
  // (Where the 16-byte path exists an interior tile also needs 16-byte
  // rows, so that instantiation holds the 16-byte stores alone.)
  const bool fullN = vecOK && (!W16 || vec16OK) && (n0 + BN <= N);

  // one instantiation per cache policy and per interior/ragged: the sc1
  // (agent-scope write-through) choice and the column checks are ONE
  // block-uniform branch per epilogue, not one per store
  auto epilogue = [&](auto sc1c, auto fullc) {
    constexpr bool SC1 = decltype(sc1c)::value;
    constexpr bool FULL = decltype(fullc)::value;
    // 16-byte stores. A lane holds columns cq..cq+3 of every fragment; a
    // fragment pair (x, y) exchanges its packed dwords with
    // v_permlane16_swap (x's odd 16-lane rows <-> y's even rows), after
    // which 16-lane group g holds the EIGHT consecutive columns
    // 8*(g>>1)..+7 of fragment x + (g&1): one 16-byte store per pair
    // instead of two 8-byte ones. Values are converted before the swap,
    // so the stored bits are those of the 8-byte path. Plain stores only:
    // the sc1 word stays 8 bytes (the widest agent-scope write-through
    // store), and a single packed output (gated BN=128) has no pair.
    if constexpr (!SC1 && W16) {
      if (FULL || vec16OK) {  // an interior tile implies vec16OK here
        const int g4 = lane >> 4;
        const int nOut = GATED ? (N >> 1) : N;
        // first of this lane's eight columns in pair 0
        const int col8 = (GATED ? (n0 >> 1) + wc * (BN / 8)
                                : n0 + wc * (BN / 4)) +
                         (g4 & 1) * 16 + (g4 >> 1) * 8;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          const int row = wr * (BM / 2) + mi * 16 + rl16;
          const int m = m0 + row;
          OT* orow;
          float rowScale = 1.0f;
          if constexpr (PHASE == 1) {
            const TPS tp = sTps[row];  // {0, 1.0f} for rows past routed
            if (slot) {
              orow = outBase + ((size_t)tpsTok(tp.tokenIdx) * nSlot +
                                tpsJ(tp.tokenIdx)) * rowPitch;
              if (scaled) rowScale = sScale[row];
            } else {
              orow = outBase + (size_t)tpsTok(tp.tokenIdx) * rowPitch;
            }
          } else {
            orow = outBase + (size_t)m * rowPitch;
          }
          uint32_t w[NOUT][2];
#pragma unroll
          for (int no = 0; no < NOUT; ++no) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              if constexpr (GATED) {
                v[r] = gate_act(accS(mi, 2 * no, r), act) *
                       accS(mi, 2 * no + 1, r);
              } else {
                v[r] = accS(mi, no, r) + bv[no][r];
                if constexpr (PHASE == 0)
                  v[r] = (act == 0)
                      ? fmaxf(v[r], 0.0f)
                      : 0.5f * v[r] *
                            (1.0f + erff(v[r] * 0.70710678118654752f));
                if constexpr (PHASE == 1)
                  if (slot) v[r] = v[r] * rowScale;
              }
            }
            w[no][0] = ETr<ET>::pack2(v[0], v[1]);
            w[no][1] = ETr<ET>::pack2(v[2], v[3]);
          }
          // the swaps run under full EXEC, ahead of the row predicate
#pragma unroll
          for (int no = 0; no < NOUT; no += 2)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const auto sw = __builtin_amdgcn_permlane16_swap(
                  w[no][h], w[no + 1][h], false, false);
              w[no][h] = sw[0];
              w[no + 1][h] = sw[1];
            }
          if ((uint32_t)m >= routed) continue;  // rows past routed
#pragma unroll
          for (int no = 0; no < NOUT; no += 2) {
            const int c = col8 + no * 16;
            const int nValid = FULL ? 8 : nOut - c;  // columns >= N: not written
            if (!FULL && nValid <= 0) continue;
            const uint32_t ww[4] = {w[no][0], w[no][1], w[no + 1][0],
                                    w[no + 1][1]};
            storeRow8(orow + c, ww, nValid);
          }
        }
        return;
      }
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const int row = wr * (BM / 2) + mi * 16 + rl16;
      const int m = m0 + row;
      if ((uint32_t)m >= routed) continue;  // rows past routed: not written
      OT* orow;
      float rowScale = 1.0f;
      if constexpr (PHASE == 1) {
        const TPS tp = sTps[row];
        if (slot) {
          // non-atomic per-(token, j) combine slot (summed with the
          // kept mask in k_cast_combine; replaces fp32 atomics)
          orow = outBase + ((size_t)tpsTok(tp.tokenIdx) * nSlot +
                            tpsJ(tp.tokenIdx)) * rowPitch;
          if (scaled) rowScale = sScale[row];
        } else {
          orow = outBase + (size_t)tpsTok(tp.tokenIdx) * rowPitch;
        }
      } else {
        orow = outBase + (size_t)m * rowPitch;
      }
      if constexpr (GATED) {
        // fragment pairs: accv[mi][2j] is g and accv[mi][2j+1] is u for
        // P columns col0..col0+3; act(g) * u in fp32, rounded once by the
        // store. The tile covers BN/2 P-columns from n0/2; a tile that is
        // full in the effective N is full in P too.
        const int P = N >> 1;
        const int pBase = (n0 >> 1) + wc * (BN / 8) + cq;
#pragma unroll
        for (int j = 0; j < NF / 2; ++j) {
          const int col0 = pBase + j * 16;
          const int nValid = FULL ? 4 : P - col0;
          if (!FULL && nValid <= 0) continue;
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r)
            v[r] = gate_act(accS(mi, 2 * j, r), act) * accS(mi, 2 * j + 1, r);
          storeRow4<SC1>(orow + col0, v, nValid, FULL || vecOK);
        }
        continue;
      }
#pragma unroll
      for (int ni = 0; ni < NF; ++ni) {
        const int col0 = nBase + ni * 16;
        // columns >= N are not written
        const int nValid = FULL ? 4 : N - col0;
        if (!FULL && nValid <= 0) continue;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = accS(mi, ni, r) + bv[ni][r];
          if constexpr (PHASE == 0)
            v[r] = (act == 0)
                ? fmaxf(v[r], 0.0f)
                : 0.5f * v[r] * (1.0f + erff(v[r] * 0.70710678118654752f));
          if constexpr (PHASE == 1)
            if (slot) v[r] = v[r] * rowScale;
        }
        if constexpr (PHASE == 3) {
          // gate logits, fp32; atomic accumulate when the fused gate
          // K-splits the logits GEMM over jobs (logits32 kept zero
          // between forwards by the route's re-zeroing pass)
          if (a.atomicLogits) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (r < nValid) atomicAdd(orow + col0 + r, v[r]);
          } else if (FULL || (vecOK && nValid >= 4)) {
            *reinterpret_cast<f32x4*>(orow + col0) =
                f32x4{v[0], v[1], v[2], v[3]};
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (r < nValid) orow[col0 + r] = v[r];
          }
        } else {
          // PHASE 0 / PHASE 1 carry the sc1 policy (in-launch consumers
          // in the fused kernel); PHASE 2 is always a plain store
          storeRow4<SC1 && (PHASE == 0 || PHASE == 1)>(orow + col0, v,
                                                        nValid, FULL || vecOK);
        }
      }
    }
  };
  constexpr bool CAN_SC1 = RT_SC1 && (PHASE == 0 || PHASE == 1);
  const bool sc1 = CAN_SC1 && a.sc1Out != 0;
  if (sc1 && fullN) epilogue(BoolC<CAN_SC1>{}, BoolC<true>{});
  else if (sc1) epilogue(BoolC<CAN_SC1>{}, BoolC<false>{});
  else if (fullN) epilogue(BoolC<false>{}, BoolC<true>{});
  else epilogue(BoolC<false>{}, BoolC<false>{});
  FM_STAMP(3);
#ifdef FM_GEMM_STAMPS
  {
    const int blk =
        blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    if (tid == 0 && blk < FM_STAMP_BLOCKS && jobLocal < FM_STAMP_JOBS)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        g_gemmStamps[PHASE][blk][jobLocal][i] = fmStamp[i];
  }
#endif
  return true;
}

// ---------------------------------------------------------------------------
// Big-tile grouped GEMM kernel (classic multi-kernel path): XCD-aware
// remap loop around gemm_job_body. See the body above for the tile
// pipeline; DESIGN.md par.3 for the mode selection.
// ---------------------------------------------------------------------------
template <typename ET, int PHASE, int ACT, bool HAS_BIAS, int BN, int BM = 256,
          typename WET = ET, int STAGES = 2>
__global__ __launch_bounds__(512, 2) void k_group_gemm_bf16_big(GemmArgs a) {
  constexpr int BEZ = (int)sizeof(WET);
  __shared__ __attribute__((aligned(16))) char smem[
      gemm_lds_bytes<BM, BN, BEZ, STAGES>()];

  // XCD-aware block remap (perf only, placement-independent for
  // correctness): the dispatcher places linear block b on XCD b%8; the
  // bijective remap gives each XCD a CONTIGUOUS chunk of (e, nTile)
  // space with mTile fastest, so the blocks sharing a B weight panel
  // (and, for small E, a whole expert) run on one XCD and hit its L2
  // instead of re-reading HBM/L3 (guide T1; staging-traffic-bound at
  // 6.2 TB/s before this, profiles/r01 pmc2).
  const int mT = a.totalJobs > 0 ? a.jobsMT : gridDim.x;
  const int nT = a.totalJobs > 0 ? a.jobsNT : gridDim.y;
  const int gstride = gridDim.x * gridDim.y * gridDim.z;
  const int nBlocks = a.totalJobs > 0 ? a.totalJobs : gstride;
  const int lin0 =
      blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  const int qx = nBlocks / 8, rx = nBlocks % 8;
  const int sk = a.splitK > 0 ? a.splitK : 1;
  const int zE = (a.totalJobs > 0 ? a.totalJobs / (mT * nT)
                                  : (int)gridDim.z) / sk;
  // persistent grid (totalJobs > 0): each block walks jobs lin0,
  // lin0+gstride, ... - the per-launch block setup (sTps load, source
  // pointer setup, I$ warm, prologue staging bubble) amortizes over
  // several tiles instead of being paid once per 16-tile block
  // (mfma_probe: the identical tile loop runs 52.5 us/forward-equiv
  // persistent vs 71.4 us launched per-tile at the cfg2 up shape)
  int par = 0;  // metadata copy; flips after every job that ran
  for (int jl = lin0; jl < nBlocks; jl += gstride) {
    const int xcd = jl % 8, pos = jl / 8;
    const int swz = a.noRemap
        ? jl
        : (xcd < rx ? xcd * (qx + 1) : rx * (qx + 1) + (xcd - rx) * qx) + pos;
    const int eEff = swz / (mT * nT);  // in [0, E*splitK)
    const int e = eEff % zE;
    const int ksplit = eEff / zE;
    const int rem = swz % (mT * nT);
    // ACT 2/3 (PHASE 0 only) select the gated body; every other
    // instantiation is the ungated code unchanged
    const bool ran = gemm_job_body<ET, PHASE, BN, BM, WET, STAGES, 0, 0, false,
                                   (PHASE == 0 && ACT >= 2)>(
        a, smem, e, ksplit, (rem % mT) * BM, (rem / mT) * BN, ACT, HAS_BIAS,
        par, (jl - lin0) / gstride);
    par ^= ran ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------
// MX-fp8 grouped GEMM (dtype 5): fp8 e4m3 A (runtime-quantized
// activations, per-64-element E8M0 scales) x fp8 e4m3 B (expert weights,
// scale 1) on v_mfma_scale_f32_16x16x128_f8f6f4 - the 2x-rate CDNA4
// path (~4.7 PF/s vs 2.5 bf16). 128x128 tile, BK=128 (one scaled MFMA
// covers the whole K-tile), 512 threads = 8 waves (2M x 4N), fp32
// accumulate, bf16 outputs. Staging geometry is byte-identical to the
// bf16 kernel's (128-B rows, XOR-16B-chunk swizzle, glds double
// buffer); A/B bytes per K-element halve, so HBM/LDS traffic halves
// too. Scale->lane mapping empirically pinned by
// test_mx_mfma_layout_probe: lane-group g's scale byte covers
// k in [64g, 64g+64) (opsel selects the byte; groups 2..3 unused).
// PHASE semantics match gemm_job_body (0 up / 1 down+slots / 2 packed).
// ---------------------------------------------------------------------------

#define MI_OF(BMV) ((BMV) / 32)
template <int PHASE, int BM = 128, int BN = 128, int STAGES = 2>
__device__ __forceinline__ bool mx_gemm_job_body(
    const GemmArgs& a, char* smemBase, int e, int m0, int n0, int act,
    bool hasBias) {
  constexpr int BK = 128;
  // triple buffering (SE=3) gives each stage TWO compute phases of
  // latency budget (the 2-stage pipeline's per-tile vmcnt(0) drain is
  // the measured stall: MFMA pipe ~12%, profiles/r02_mx_pmc.txt);
  // degrade when it would not fit LDS
  constexpr int SE =
      (STAGES == 3 && 3 * (BM + BN) * BK + BM * 8 + 16 > 160 * 1024)
          ? 2 : STAGES;
  uint8_t* Abase = reinterpret_cast<uint8_t*>(smemBase);   // SE x [BM][BK]
  uint8_t* Bbase = reinterpret_cast<uint8_t*>(smemBase + SE * BM * BK);
  TPS* sTps = reinterpret_cast<TPS*>(smemBase + SE * BM * BK + SE * BN * BK);
  uint32_t* sRouted = reinterpret_cast<uint32_t*>(sTps + BM);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int K = a.K, N = a.N;

  const TPS* tpsE = a.tokenIds ? a.tokenIds + (size_t)e * a.pEC : nullptr;
  __syncthreads();  // prior job's LDS readers done
  if (tid == 0)
    *sRouted = tpsE ? min(a.eC[e], (uint32_t)a.EC) : (uint32_t)a.nRows;
  __syncthreads();
  const uint32_t routed = *sRouted;
  if ((uint32_t)m0 >= routed) return false;
  const int mCap = a.tokenIds ? a.pEC : a.nRows;
  const int we = a.segExpert ? a.segExpert[e] : e;
  if (tid < BM) {
    TPS t{0u, 1.0f};
    if ((uint32_t)(m0 + tid) < routed)
      t = tpsE ? tpsE[m0 + tid] : TPS{(uint32_t)(m0 + tid), 1.0f};
    sTps[tid] = t;
  }
  __syncthreads();

  const uint8_t* __restrict__ Ag = reinterpret_cast<const uint8_t*>(a.A);
  const uint8_t* __restrict__ Bg =
      reinterpret_cast<const uint8_t*>(a.B) + (size_t)we * a.strideBExpert;
  const uint8_t* __restrict__ aS =
      reinterpret_cast<const uint8_t*>(a.aScales);

  // glds staging: 16 KiB per operand tile = 16 x 1 KiB groups (8 rows of
  // 128 B each); lane -> (row-in-group = lane/8, 16B chunk = lane%8),
  // chunk XOR-swizzled by row for conflict-free b128 fragment reads
  const int grow8 = lane >> 3;
  const int schunk = (lane & 7) ^ grow8;
  constexpr int GPW_A = BM / 8 / 8;  // 1 KiB glds groups per wave (A)
  constexpr int GPW_B = BN / 8 / 8;
  const size_t aBase = (size_t)e * a.strideAExpert;  // bytes (u8 A)
  const uint8_t* aSrc[GPW_A];
  const uint8_t* bSrc[GPW_B];
#pragma unroll
  for (int i = 0; i < GPW_A; ++i) {
    const int row = (wave * GPW_A + i) * 8 + grow8;
    const size_t arow = (PHASE == 0) ? (size_t)tpsTok(sTps[row].tokenIdx)
                                     : (size_t)min(m0 + row, mCap - 1);
    aSrc[i] = Ag + aBase + arow * (size_t)K + schunk * 16;
  }
#pragma unroll
  for (int i = 0; i < GPW_B; ++i) {
    const int row = (wave * GPW_B + i) * 8 + grow8;
    bSrc[i] = Bg + (size_t)min(n0 + row, N - 1) * K + schunk * 16;
  }
  auto stage = [&](int kt, int buf) {
#pragma unroll
    for (int i = 0; i < GPW_A; ++i)
      __builtin_amdgcn_global_load_lds(
          (gas_u32*)(aSrc[i] + kt),
          (las_u32*)(Abase + buf * BM * BK + (wave * GPW_A + i) * 1024), 16,
          0, 0);
#pragma unroll
    for (int i = 0; i < GPW_B; ++i)
      __builtin_amdgcn_global_load_lds(
          (gas_u32*)(bSrc[i] + kt),
          (las_u32*)(Bbase + buf * BN * BK + (wave * GPW_B + i) * 1024), 16,
          0, 0);
  };

  // wave grid 2(M) x 4(N): BM/2 rows x BN/4 cols per wave
  const int wr = wave >> 2, wc = wave & 3;
  constexpr int MI = BM / 32, NF = BN / 64;
  f32x4 accv[MI][NF];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) accv[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // per-lane fragment geometry: row rl, k-group g (32 elements each);
  // the lane's SCALE byte must be the contiguous-64-block (g & 1)'s
  // scale (hardware maps scale-group g to the interleaved chunk pair
  // {k>>6 == g&1, (k>>4)&1 == g>>1} - pinned by the MX layout probe)
  const int rl = lane & 15;
  const int gk = lane >> 4;
  const int K64 = K / 64;

  // per-lane A-scale source rows (this lane's 4 fragment rows), hoisted
  const uint8_t* sRow[MI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int R = wr * (BM / 2) + mi * 16 + rl;
    const size_t arow = (PHASE == 0) ? (size_t)tpsTok(sTps[R].tokenIdx)
                                     : (size_t)min(m0 + R, mCap - 1);
    sRow[mi] = aS + (aBase / 64) + arow * K64 + (gk & 1);
  }
  const int nK = K / BK;
  // counted end-of-tile wait: with SE=3, tile t+1 must have landed but
  // tile t+2's GPT glds AND the MI prefetched scale-byte loads (issued
  // after them, completing in order) may stay in flight
  constexpr int GPW_AB = GPW_A + GPW_B;
  constexpr int WN3 = (GPW_AB + MI_OF(BM) <= 10) ? 10 : 12;
  stage(0, 0);
  // software-pipelined scale bytes: tile t's scattered global byte
  // loads are issued one tile AHEAD so they never sit on the MFMA
  // dependency chain
  int sav[MI], savNext[MI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) sav[mi] = sRow[mi][0];
  if constexpr (SE == 3) {
    if (nK > 1) {
      stage(BK, 1);
      wait_vmcnt<GPW_AB>();  // tile 0 landed; tile 1 in flight
    } else {
      wait_vmcnt<0>();
    }
  } else {
    wait_vmcnt<0>();
  }
  __builtin_amdgcn_s_barrier();
  for (int t = 0; t < nK; ++t) {
    const int pre = t + SE - 1;      // tile staged this iteration
    const bool stageNow = pre < nK;
    if (stageNow) stage(pre * BK, pre % SE);
    if (t + 1 < nK) {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) savNext[mi] = sRow[mi][(t + 1) * 2];
    }
    const uint8_t* Al = Abase + (t % SE) * BM * BK;
    const uint8_t* Bl = Bbase + (t % SE) * BN * BK;
    __builtin_amdgcn_s_setprio(1);
    i32x8 af[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const int R = wr * (BM / 2) + mi * 16 + rl;
      const int c0 = (2 * gk) ^ (R & 7);
      const int c1 = (2 * gk + 1) ^ (R & 7);
      const u32x4 lo = *reinterpret_cast<const u32x4*>(&Al[R * BK + c0 * 16]);
      const u32x4 hi = *reinterpret_cast<const u32x4*>(&Al[R * BK + c1 * 16]);
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        af[mi][d] = (int)lo[d];
        af[mi][4 + d] = (int)hi[d];
      }
    }
    i32x8 bfr[NF];
#pragma unroll
    for (int ni = 0; ni < NF; ++ni) {
      const int R = wc * (BN / 4) + ni * 16 + rl;
      const int c0 = (2 * gk) ^ (R & 7);
      const int c1 = (2 * gk + 1) ^ (R & 7);
      const u32x4 lo = *reinterpret_cast<const u32x4*>(&Bl[R * BK + c0 * 16]);
      const u32x4 hi = *reinterpret_cast<const u32x4*>(&Bl[R * BK + c1 * 16]);
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        bfr[ni][d] = (int)lo[d];
        bfr[ni][4 + d] = (int)hi[d];
      }
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NF; ++ni)
        accv[mi][ni] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            af[mi], bfr[ni], accv[mi][ni], 0 /*fp8*/, 0 /*fp8*/, 0, sav[mi],
            0, 0x7F /*B scale 1.0*/);
    __builtin_amdgcn_s_setprio(0);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) sav[mi] = savNext[mi];
    if constexpr (SE == 3) {
      if (stageNow) wait_vmcnt<WN3>(); else wait_vmcnt<0>();
    } else {
      wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();
  }

  // epilogue (bf16 outputs; mirrors gemm_job_body's PHASE semantics)
  const int cl = lane & 15;
  const int r0 = (lane >> 4) * 4;
  float* sScale = reinterpret_cast<float*>(Abase);
  const bool slot = (PHASE == 1) && (a.topk > 1 || a.slotAlways);
  const bool scaled = (PHASE == 1) && a.topk > 1;
  if constexpr (PHASE == 1) {
    if (scaled) {
      __syncthreads();
      if (tid < BM) {
        const TPS tp = sTps[tid];
        float sc = 0.0f;
        if ((uint32_t)(m0 + tid) < routed)
          sc = toF(reinterpret_cast<const bf16*>(
                   a.gate_out)[(size_t)tpsTok(tp.tokenIdx) * a.PX +
                               a.expertOffset + e]) / tp.probSum;
        sScale[tid] = sc;
      }
      __syncthreads();
    }
  }
  float bv[NF];
#pragma unroll
  for (int ni = 0; ni < NF; ++ni) bv[ni] = 0.f;
  if (hasBias) {
    const bf16* bptr = reinterpret_cast<const bf16*>(a.bias) +
                       (a.strideBExpert ? (size_t)we * N : 0);
#pragma unroll
    for (int ni = 0; ni < NF; ++ni) {
      const int col = n0 + wc * (BN / 4) + ni * 16 + cl;
      if (col < N) bv[ni] = toF(bptr[col]);
    }
  }
  // per-column weight scales of this job (1.0f without scales), beside bv
  float sv[NF];
  {
    const float* sp =
        a.wScale ? a.wScale + (size_t)we * a.wScaleStride : nullptr;
#pragma unroll
    for (int ni = 0; ni < NF; ++ni)
      sv[ni] = wscale_at(sp, n0 + wc * (BN / 4) + ni * 16 + cl, N);
  }
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wr * (BM / 2) + mi * 16 + r0 + r;
      const int m = m0 + row;
      if ((uint32_t)m >= routed) continue;
      const TPS tp = sTps[row];
      const float rowScale = scaled ? sScale[row] : 1.0f;
#pragma unroll
      for (int ni = 0; ni < NF; ++ni) {
        const int col = n0 + wc * (BN / 4) + ni * 16 + cl;
        if (col >= N) continue;
        float v = accv[mi][ni][r] * sv[ni] + bv[ni];
        if constexpr (PHASE == 0) {
          v = (act == 0) ? fmaxf(v, 0.0f)
                         : 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
          if (!(a.out8 && BN == 256))
            reinterpret_cast<bf16*>(a.out)[(size_t)e * a.strideOExpert +
                                           (size_t)m * N + col] =
                __float2bfloat16(v);
        } else if constexpr (PHASE == 1) {
          if (slot) {
            reinterpret_cast<bf16*>(a.O32)[
                ((size_t)tpsTok(tp.tokenIdx) * a.topk + tpsJ(tp.tokenIdx)) *
                    a.H + col] = __float2bfloat16(v * rowScale);
          } else {
            reinterpret_cast<bf16*>(
                a.moe_out)[(size_t)tpsTok(tp.tokenIdx) * a.H + col] =
                __float2bfloat16(v);
          }
        } else {
          reinterpret_cast<bf16*>(a.out)[(size_t)e * a.strideOExpert +
                                         (size_t)m * N + col] =
              __float2bfloat16(v);
        }
      }
    }
  }
  if constexpr (PHASE == 0 && BN == 256) {
    if (a.out8) {
      // epilogue MX quantization: each quarter-wave (16 lanes x NF=4
      // cols each) holds exactly ONE contiguous 64-col block of a row.
      // bf16-round first (the CPU restatement Element-rounds the
      // intermediate before quantizing), 16-lane blockmax, E8M0 scale,
      // e4m3 RNE pack via v_cvt_pk_fp8_f32.
      uint8_t* o8 = reinterpret_cast<uint8_t*>(a.out8) +
                    (size_t)e * a.strideOExpert;
      uint8_t* oS = reinterpret_cast<uint8_t*>(a.outScales) +
                    (size_t)e * (a.strideOExpert / 64);
      const int blk = n0 / 64 + wc;  // this quarter-wave's 64-block
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = wr * (BM / 2) + mi * 16 + r0 + r;
          const int m = m0 + row;
          if ((uint32_t)m >= routed) continue;
          float vq[NF];
          float mx = 0.0f;
#pragma unroll
          for (int ni = 0; ni < NF; ++ni) {
            float v = accv[mi][ni][r] * sv[ni] + bv[ni];
            v = (act == 0)
                    ? fmaxf(v, 0.0f)
                    : 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
            vq[ni] = __bfloat162float(__float2bfloat16(v));
            mx = fmaxf(mx, fabsf(vq[ni]));
          }
#pragma unroll
          for (int off = 1; off < 16; off <<= 1)
            mx = fmaxf(mx, __shfl_xor(mx, off, 16));
          int eE = 0;
          if (mx > 0.0f) {
            int ex;
            (void)frexpf(mx / 448.0f, &ex);
            eE = ex < -126 ? -126 : (ex > 127 ? 127 : ex);
          }
          const float inv = exp2f((float)-eE);
          const uint32_t p01 = cvt2_fp8(vq[0] * inv, vq[1] * inv);
          const uint32_t p23 = cvt2_fp8(vq[2] * inv, vq[3] * inv);
          uint8_t* orow = o8 + (size_t)m * N;
#pragma unroll
          for (int ni = 0; ni < NF; ++ni) {
            const int col = n0 + wc * (BN / 4) + ni * 16 + cl;
            const uint32_t src = (ni < 2) ? p01 : p23;
            orow[col] = (uint8_t)((src >> ((ni & 1) * 8)) & 0xFF);
          }
          if (cl == 0)
            oS[(size_t)m * (N / 64) + blk] = (uint8_t)(127 + eE);
        }
      }
    }
  }
  return true;
}

template <int PHASE, int ACT, bool HAS_BIAS, int BM = 128, int BN = 128,
          int STAGES = 2>
__global__ __launch_bounds__(512, 2) void k_group_gemm_mx(GemmArgs a) {
  constexpr int BK = 128;
  constexpr int SE =
      (STAGES == 3 && 3 * (BM + BN) * BK + BM * 8 + 16 > 160 * 1024)
          ? 2 : STAGES;
  __shared__ __attribute__((aligned(16))) char smem[
      SE * BM * BK + SE * BN * BK + BM * 8 + 16];
  const int mT = a.totalJobs > 0 ? a.jobsMT : gridDim.x;
  const int nT = a.totalJobs > 0 ? a.jobsNT : gridDim.y;
  const int gstride = gridDim.x * gridDim.y * gridDim.z;
  const int nBlocks = a.totalJobs > 0 ? a.totalJobs : gstride;
  const int lin0 =
      blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  const int qx = nBlocks / 8, rx = nBlocks % 8;
  for (int jl = lin0; jl < nBlocks; jl += gstride) {
    const int xcd = jl % 8, pos = jl / 8;
    const int swz = a.noRemap
        ? jl
        : (xcd < rx ? xcd * (qx + 1) : rx * (qx + 1) + (xcd - rx) * qx) + pos;
    const int e = swz / (mT * nT);
    const int rem = swz % (mT * nT);
    (void)mx_gemm_job_body<PHASE, BM, BN, STAGES>(
        a, smem, e, (rem % mT) * BM, (rem / mT) * BN, ACT, HAS_BIAS);
  }
}

// ---------------------------------------------------------------------------
// fp32 grouped GEMM (config-1 "CPU correctness plumbing" shapes; VALU
// tiled). 64x64 tile, 256 threads, each thread a 4x4 sub-block, BK=16.
// Same phase semantics as the bf16 kernel.
// ---------------------------------------------------------------------------

template <int PHASE, int ACT, bool HAS_BIAS>
__global__ __launch_bounds__(256) void k_group_gemm_f32(GemmArgs a) {
  constexpr int BM = 64, BN = 64, BK = 16;
  constexpr bool GATED = (PHASE == 0) && (ACT >= 2);
  constexpr int LDT = BK + 1;
  __shared__ float Alds[BM * LDT];
  __shared__ float Blds[BN * LDT];
  __shared__ TPS sTps[BM];
  __shared__ uint32_t sRouted;

  const int e = blockIdx.z;
  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int K = a.K, N = a.N;
  const TPS* tpsE = a.tokenIds ? a.tokenIds + (size_t)e * a.pEC : nullptr;
  const int we = a.segExpert ? a.segExpert[e] : e;
  if (tid == 0)
    sRouted = tpsE ? min(a.eC[e], (uint32_t)a.EC) : (uint32_t)a.nRows;
  __syncthreads();
  const uint32_t routed = sRouted;
  if ((uint32_t)m0 >= routed) return;
  if (tid < BM) {
    TPS t{0u, 1.0f};
    if ((uint32_t)(m0 + tid) < routed)
      t = tpsE ? tpsE[m0 + tid] : TPS{(uint32_t)(m0 + tid), 1.0f};
    sTps[tid] = t;
  }
  __syncthreads();

  const float* __restrict__ Ag = reinterpret_cast<const float*>(a.A);
  const float* __restrict__ Bg =
      reinterpret_cast<const float*>(a.B) + (size_t)we * a.strideBExpert;

  const int tr = (tid / 16) * 4;  // thread rows [tr, tr+4)
  const int tc = (tid % 16) * 4;
  float acc[4][4] = {};
  for (int kt = 0; kt < K; kt += BK) {
    // stage: BM*BK = 1024 floats, 256 threads x 4
#pragma unroll
    for (int u4 = 0; u4 < 4; ++u4) {
      const int u = tid + u4 * 256;
      const int row = u / BK, cc = u % BK;
      const float* src = (PHASE == 0)
          ? Ag + (size_t)tpsTok(sTps[row].tokenIdx) * a.H + kt + cc
          : Ag + (size_t)e * a.strideAExpert + (size_t)(m0 + row) * K + kt + cc;
      Alds[row * LDT + cc] = *src;
      if constexpr (GATED) {
        // row-interleaved source: even tile rows read Wglu, odd ones Wup,
        // at P row (n0 + row) / 2; clamp per half (N is 2P here)
        const int prow = min((n0 + row) >> 1, (N >> 1) - 1);
        const float* bexp = (row & 1) ? Bg : Bg + a.gluOffset;
        Blds[row * LDT + cc] = bexp[(size_t)prow * K + kt + cc];
      } else {
        const int brow = min(n0 + row, N - 1);
        Blds[row * LDT + cc] = Bg[(size_t)brow * K + kt + cc];
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < BK; ++kk) {
      float av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) av[i] = Alds[(tr + i) * LDT + kk];
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = Blds[(tc + j) * LDT + kk];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
    }
    __syncthreads();
  }

  // multi / scaled / nSlot: as in the 128^2 kernel (shared-expert slices
  // write their slot unscaled)
  const bool multi = (PHASE == 1) && (a.topk > 1 || a.slotAlways);
  const bool scaled =
      (PHASE == 1) && a.topk > 1 && !(a.nShared && e >= a.nRoutedE);
  const int nSlot = a.topk + a.nShared;
  float bv[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (HAS_BIAS) {
    // per-expert bias slabs when multi-expert (see the 128^2 kernel)
    const float* bptr = reinterpret_cast<const float*>(a.bias) +
                        (a.strideBExpert ? (size_t)we * N : 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = n0 + tc + j;
      if (col < N) bv[j] = bptr[col];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + tr + i;
    if ((uint32_t)m >= routed) continue;
    const TPS tp = sTps[tr + i];
    float rowScale = 1.0f;
    if (scaled)
      rowScale = reinterpret_cast<const float*>(
                     a.gate_out)[(size_t)tpsTok(tp.tokenIdx) * a.PX +
                                 a.expertOffset + e] / tp.probSum;
    if constexpr (GATED) {
      // column pairs (2j, 2j+1) hold (g, u) of the same (row, p)
      const int P = N >> 1;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = ((n0 + tc) >> 1) + j;
        if (col >= P) continue;
        reinterpret_cast<float*>(a.out)[(size_t)e * a.strideOExpert +
                                        (size_t)m * P + col] =
            gate_act(acc[i][2 * j], ACT) * acc[i][2 * j + 1];
      }
      continue;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = n0 + tc + j;
      if (col >= N) continue;
      float v = acc[i][j] + bv[j];
      if constexpr (PHASE == 0) {
        v = (ACT == 0) ? fmaxf(v, 0.0f)
                       : 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
        reinterpret_cast<float*>(a.out)[(size_t)e * a.strideOExpert +
                                        (size_t)m * N + col] = v;
      } else if constexpr (PHASE == 1) {
        if (multi) {
          reinterpret_cast<float*>(a.O32)[
              ((size_t)tpsTok(tp.tokenIdx) * nSlot + tpsJ(tp.tokenIdx)) *
                  a.H + col] = v * rowScale;
        } else {
          reinterpret_cast<float*>(
              a.moe_out)[(size_t)tpsTok(tp.tokenIdx) * a.H + col] = v;
        }
      } else {
        reinterpret_cast<float*>(a.out)[(size_t)e * a.strideOExpert +
                                        (size_t)m * N + col] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Weight-streaming expert FFN for decode-sized forwards (S < 128, bf16 /
// fp16 / fp8 weights). An expert sees a handful of rows,
// so the forward is bound by streaming the weights of the experts that were
// hit once. One block = 16 weight rows (output columns) of one z-slice; its
// four waves split K in interleaved 128-element chunks and sum their
// partials through LDS in wave order (no atomics: the result is a pure
// function of the inputs). A slice without rows returns before it touches a
// weight.
//   weights      straight from global memory into the MFMA B fragment, 16 B
//                per lane, K-contiguous (fp8: 16 bytes = two K-steps of one
//                lane, dequantised at fragment use); the next chunk's loads
//                are issued before the current chunk is consumed (two named
//                register sets, so the compiler's waits stay counted)
//   activations  the expert's rows (x gathered through tokenIds, or xM) are
//                L2-resident and re-read by every block of the slice: each
//                wave stages its chunk in full 256-B row pieces into its own
//                LDS region and reads A fragments with 16-B LDS loads
//   rows         up to kDecRows = 32 per pass (two 16-row fragments sharing
//                each loaded B fragment); more rows take further passes
// PHASE 0 (up; GATED streams the Wglu and Wup rows of the same P range and
// stores act(g) * u), PHASE 1 (down) with the combine epilogue of
// gemm_job_body PHASE 1. Consumes the same GemmArgs routing metadata; N is
// the plain output width (P or H) and gluOffset the Wup -> Wglu distance.
// ---------------------------------------------------------------------------
constexpr int kDecBK = 128;          // K elements per staged chunk
constexpr int kDecLDA = kDecBK + 8;  // LDS row pitch in elements (272 B)
constexpr int kDecRows = 32;         // rows per pass
// unset FM_DECODE_FFN: the streaming kernels are the default up to the
// largest S at which every one of their measured runs beat every run of the
// grouped GEMMs on all three model shapes (DESIGN.md par.5k has the A/B):
// bf16 S <= 4, fp16 S <= 8 (measured at 1, 2, 4, 8), fp8 weights S <= 16.
// Above, the default stays the grouped GEMMs.
constexpr int kDecodeFfnMaxSBf16 = 4;
constexpr int kDecodeFfnMaxSFp16 = 8;
constexpr int kDecodeFfnMaxSFp8 = 16;

// WS (fp8 weights only): a.wScale is set and the epilogue applies the
// per-output-channel weight scales. A template flag, not a
// run-time test of the pointer: with the test, a forward WITHOUT scales
// measured 1.4 us slower than the parent at S = 4, outside the parent's own
// range. WS = false is the parent's kernel. The ungated fp8 kernels sit at
// the register count of four waves per SIMD (LDS allows four blocks per CU);
// the floor keeps the allocator there for their WS siblings, whose epilogue
// carries one more value. Every other instantiation keeps the default.
template <typename ET, typename WET, int PHASE, bool GATED, bool WS = false>
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu((WS && !GATED) ? 4 : 1)))
void k_decode_ffn(GemmArgs a) {
  using vec8 = typename ETr<ET>::vec8;
  constexpr int BEZ = (int)sizeof(WET);
  constexpr int KPL = 16 / BEZ;               // K elements per 16-B load
  constexpr int NLD = kDecBK / (4 * KPL);     // loads per chunk and matrix
  constexpr int NM = GATED ? 2 : 1;           // 0: Wup (or the one matrix)
  constexpr int kArena = 4 * kDecRows * kDecLDA * 2;
  __shared__ __attribute__((aligned(16))) char smem[128 * 8 + kArena];
  TPS* sTps = reinterpret_cast<TPS*>(smem);
  f32x4* red = reinterpret_cast<f32x4*>(smem + 128 * 8);  // overlays A

  const int e = blockIdx.y;
  const uint32_t routed = min(a.eC[e], (uint32_t)min(a.EC, 128));
  if (routed == 0) return;  // before any weight is touched

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int q = lane >> 4;    // K sub-range of the lane within a load
  const int rl = lane & 15;   // fragment row (A) / weight row (B)
  const int K = a.K, N = a.N;
  const int n0 = blockIdx.x * 16;
  const int we = a.segExpert ? a.segExpert[e] : e;  // weight / bias expert
  ET* Aw = reinterpret_cast<ET*>(smem + 128 * 8) + wave * kDecRows * kDecLDA;

  if (tid < 128) {
    TPS t{0u, 1.0f};
    if ((uint32_t)tid < routed) t = a.tokenIds[(size_t)e * a.pEC + tid];
    sTps[tid] = t;
  }
  __syncthreads();

  const ET* __restrict__ Ag = reinterpret_cast<const ET*>(a.A) +
                              (PHASE == 0 ? (size_t)0
                                          : (size_t)e * a.strideAExpert);
  const WET* __restrict__ Bw[NM];
  Bw[0] = reinterpret_cast<const WET*>(a.B) + (size_t)we * a.strideBExpert +
          (size_t)(n0 + rl) * K + q * KPL;
  if constexpr (GATED) Bw[1] = Bw[0] + a.gluOffset;
  // WS: the weight scale(s) of this block's column, loaded once per block by
  // the wave that runs the epilogue (s0: the one matrix / u, s1: g)
  float s0 = 1.0f, s1 = 1.0f;
  if constexpr (WS) {
    static_assert(BEZ == 1, "weight scales belong to fp8 weights");
    if (wave == 0) {
      const float* sp = a.wScale + (size_t)we * a.wScaleStride + n0 + rl;
      s0 = sp[0];
      if constexpr (GATED) s1 = sp[a.wScaleGlu];
    }
  }

  for (int mg0 = 0; mg0 < (int)routed; mg0 += kDecRows) {
    const int rp = min((int)routed - mg0, kDecRows);
    const bool two = rp > 16;  // a second 16-row fragment
    // A staging: 16 lanes x 16 B = one 256-B row piece, 4 rows per
    // instruction; element offset of the lane's piece, -1 past the rows
    int aOff[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = i * 4 + q;
      const int m = mg0 + r;
      aOff[i] = r < rp ? (PHASE == 0
                              ? (int)tpsTok(sTps[m].tokenIdx) * a.H
                              : m * K) + rl * 8
                       : -1;
    }
    f32x4 acc[NM][2];
#pragma unroll
    for (int mt = 0; mt < NM; ++mt)
#pragma unroll
      for (int f = 0; f < 2; ++f) acc[mt][f] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x4 areg[8];
    auto loadA = [&](int kc) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (i >= 4 && !two) break;
        areg[i] = u32x4{0u, 0u, 0u, 0u};
        if (aOff[i] >= 0 && kc + rl * 8 < K)
          areg[i] = *reinterpret_cast<const u32x4*>(Ag + aOff[i] + kc);
      }
    };
    auto storeA = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (i >= 4 && !two) break;
        *reinterpret_cast<u32x4*>(Aw + (i * 4 + q) * kDecLDA + rl * 8) =
            areg[i];
      }
    };
    auto loadB = [&](u32x4 (&b)[NM][NLD], int kc) __attribute__((always_inline)) {
#pragma unroll
      for (int mt = 0; mt < NM; ++mt)
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
          const int k = kc + j * 4 * KPL;  // wave-uniform; K % 64 == 0
          b[mt][j] = u32x4{0u, 0u, 0u, 0u};
          if (k < K) b[mt][j] = *reinterpret_cast<const u32x4*>(Bw[mt] + k);
        }
    };
    auto compute = [&](const u32x4 (&b)[NM][NLD]) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < NLD; ++j)
#pragma unroll
        for (int s = 0; s < KPL / 8; ++s) {
          const int ko = j * 4 * KPL + q * KPL + s * 8;
          const vec8 a0 =
              *reinterpret_cast<const vec8*>(Aw + rl * kDecLDA + ko);
          vec8 a1 = a0;
          if (two)
            a1 = *reinterpret_cast<const vec8*>(Aw + (16 + rl) * kDecLDA + ko);
#pragma unroll
          for (int mt = 0; mt < NM; ++mt) {
            vec8 bf;
            if constexpr (BEZ == 1)
              bf = dequant_fp8x8_bf16(b[mt][j][2 * s], b[mt][j][2 * s + 1]);
            else
              bf = __builtin_bit_cast(vec8, b[mt][j]);
            acc[mt][0] = ETr<ET>::mfma(a0, bf, acc[mt][0]);
            if (two) acc[mt][1] = ETr<ET>::mfma(a1, bf, acc[mt][1]);
          }
        }
    };
    // the A region is private to the wave: LDS serves a wave's accesses in
    // order, so a wavefront-scope fence orders its stores and fragment reads
    auto waveSync = [&]() __attribute__((always_inline)) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    };
    // consume chunk kc from bc; prefetch chunk kc + 4 * kDecBK into bn
    auto step = [&](const u32x4 (&bc)[NM][NLD], u32x4 (&bn)[NM][NLD],
                    int kc) __attribute__((always_inline)) {
      const int kn = kc + 4 * kDecBK;
      const bool more = kn < K;
      if (more) {
        loadA(kn);
        loadB(bn, kn);
      }
      compute(bc);
      if (more) {
        waveSync();
        storeA();
        waveSync();
      }
    };
    u32x4 b0[NM][NLD], b1[NM][NLD];
    const int kc0 = wave * kDecBK;
    if (kc0 < K) {
      loadA(kc0);
      loadB(b0, kc0);
      storeA();
      waveSync();
      for (int kc = kc0; kc < K; kc += 8 * kDecBK) {
        step(b0, b1, kc);
        if (kc + 4 * kDecBK < K) step(b1, b0, kc + 4 * kDecBK);
      }
    }

    // fixed-order K reduction: waves 1..3 -> LDS, wave 0 sums and stores
    __syncthreads();  // every wave is done with its A region
    if (wave > 0) {
#pragma unroll
      for (int mt = 0; mt < NM; ++mt)
#pragma unroll
        for (int f = 0; f < 2; ++f)
          red[(((wave - 1) * NM + mt) * 2 + f) * 64 + lane] = acc[mt][f];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int w = 0; w < 3; ++w)
#pragma unroll
        for (int mt = 0; mt < NM; ++mt)
#pragma unroll
          for (int f = 0; f < 2; ++f)
            acc[mt][f] += red[((w * NM + mt) * 2 + f) * 64 + lane];
      // C/D map of the 16x16 MFMA: col = lane & 15, row = (lane >> 4) * 4 + r
      const int col = n0 + rl;
      float bv = 0.0f;
      if (a.bias)
        bv = toF(reinterpret_cast<const ET*>(a.bias)[(size_t)we * N + col]);
      // WS: the reduced sums take the column's weight scale(s) in place
      // (acc[0]: the one matrix / u, acc[1]: g)
      if constexpr (WS) {
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            acc[0][f][r] *= s0;
            if constexpr (GATED) acc[1][f][r] *= s1;
          }
      }
      const bool multi = (PHASE == 1) && (a.topk > 1 || a.slotAlways);
      const bool scaled =
          (PHASE == 1) && a.topk > 1 && !(a.nShared && e >= a.nRoutedE);
      const int nSlot = a.topk + a.nShared;
#pragma unroll
      for (int f = 0; f < 2; ++f) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = f * 16 + q * 4 + r;
          if (row >= rp) continue;
          const int m = mg0 + row;
          if constexpr (PHASE == 0) {
            float v;
            if constexpr (GATED) {
              v = gate_act(acc[1][f][r], a.act) * acc[0][f][r];
            } else {
              v = acc[0][f][r] + bv;
              v = (a.act == 0)
                      ? fmaxf(v, 0.0f)
                      : 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
            }
            reinterpret_cast<ET*>(a.out)[(size_t)e * a.strideOExpert +
                                         (size_t)m * N + col] =
                ETr<ET>::fromf(v);
          } else {
            const TPS tp = sTps[m];
            const uint32_t tok = tpsTok(tp.tokenIdx);
            const float v = acc[0][f][r] + bv;
            if (multi) {
              float sc = 1.0f;
              if (scaled)
                sc = toF(reinterpret_cast<const ET*>(
                         a.gate_out)[(size_t)tok * a.PX + a.expertOffset + e]) /
                     tp.probSum;
              reinterpret_cast<ET*>(a.O32)[
                  ((size_t)tok * nSlot + tpsJ(tp.tokenIdx)) * a.H + col] =
                  ETr<ET>::fromf(v * sc);
            } else {
              reinterpret_cast<ET*>(a.moe_out)[(size_t)tok * a.H + col] =
                  ETr<ET>::fromf(v);
            }
          }
        }
      }
    }
    __syncthreads();  // the next pass restages over the reduction slabs
  }
}

// sum the k non-atomic combine slots (kept-masked) into the output
// (k>1 path; replaces the fp32-atomic accumulator + cast). Blocks walk
// token groups, 16-B vector loads per slot (a scalar grid-stride
// version with a per-element div ran at 1.35 TB/s on the cfg5 shape).
template <typename T, int K>
__global__ void k_cast_combine(const T* __restrict__ cbuf,
                               const uint8_t* __restrict__ kept,
                               T* __restrict__ out, int S, int H) {
  constexpr int EPU = 16 / sizeof(T);
  FM_AUX_STAMP(1, 0);
  // A token is H / EPU 16-byte chunks. With fewer chunks than threads
  // the block covers tpb = blockDim / chunks tokens per iteration, one
  // chunk per thread (the blockDim % chunks threads left over idle);
  // otherwise one token per iteration, threads striding over its chunks.
  // Either way every output element is one thread's sum over j in order.
  const int cpt = max(1, H / EPU);
  const int tpb = cpt < (int)blockDim.x ? (int)blockDim.x / cpt : 1;
  const int tl = tpb > 1 ? (int)threadIdx.x / cpt : 0;
  const int h0 = ((int)threadIdx.x - tl * cpt) * EPU;
  const int hStep = tpb > 1 ? H : (int)blockDim.x * EPU;
  for (int t = blockIdx.x * tpb + tl; t < S && tl < tpb;
       t += gridDim.x * tpb) {
    bool kp[K];
#pragma unroll
    for (int j = 0; j < K; ++j) kp[j] = kept[(size_t)t * K + j] != 0;
    for (int h = h0; h < H; h += hStep) {
      float acc[EPU];
#pragma unroll
      for (int q = 0; q < EPU; ++q) acc[q] = 0.0f;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (!kp[j]) continue;
        const u32x4 v = *reinterpret_cast<const u32x4*>(
            cbuf + ((size_t)t * K + j) * H + h);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const uint32_t vw = v[w];
          if constexpr (__is_same(T, bf16)) {
            const float2 f = __bfloat1622float2(
                *reinterpret_cast<const __hip_bfloat162*>(&vw));
            acc[2 * w] += f.x;
            acc[2 * w + 1] += f.y;
          } else if constexpr (__is_same(T, fp16)) {
            const float2 f = __half22float2(
                *reinterpret_cast<const __half2*>(&vw));
            acc[2 * w] += f.x;
            acc[2 * w + 1] += f.y;
          } else {
            acc[w] += __uint_as_float(vw);
          }
        }
      }
      T ov[EPU];
#pragma unroll
      for (int q = 0; q < EPU; ++q) fromF(acc[q], ov[q]);
      *reinterpret_cast<u32x4*>(out + (size_t)t * H + h) =
          *reinterpret_cast<const u32x4*>(ov);
    }
  }
  FM_AUX_STAMP(1, 1);
}

// 16 bytes of Element slots added into fp32 accumulators (the slot read
// of the shared-expert combine below)
template <typename T>
__device__ __forceinline__ void accSlot16(const T* __restrict__ p,
                                          float (&acc)[16 / sizeof(T)]) {
  const u32x4 v = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t vw = v[w];
    if constexpr (__is_same(T, bf16)) {
      const float2 f = __bfloat1622float2(
          *reinterpret_cast<const __hip_bfloat162*>(&vw));
      acc[2 * w] += f.x;
      acc[2 * w + 1] += f.y;
    } else if constexpr (__is_same(T, fp16)) {
      const float2 f = __half22float2(*reinterpret_cast<const __half2*>(&vw));
      acc[2 * w] += f.x;
      acc[2 * w + 1] += f.y;
    } else {
      acc[w] += __uint_as_float(vw);
    }
  }
}

// Sibling of k_cast_combine for num_shared_experts > 0: the slots are
// [S, K + nSh, H]; the K routed slots are kept-masked (kept is [S, K], the
// gates write it at stride K), the nSh shared slots that follow are always
// summed. fp32 sum in slot order, one rounding; same thread mapping as
// k_cast_combine. A token with every routed slot dropped still gets its
// shared terms, so K == 1 needs no zeroed moe_out either.
template <typename T, int K>
__global__ void k_cast_combine_shared(const T* __restrict__ cbuf,
                                      const uint8_t* __restrict__ kept,
                                      T* __restrict__ out, int S, int H,
                                      int nSh) {
  constexpr int EPU = 16 / sizeof(T);
  FM_AUX_STAMP(1, 0);
  const int cpt = max(1, H / EPU);
  const int tpb = cpt < (int)blockDim.x ? (int)blockDim.x / cpt : 1;
  const int tl = tpb > 1 ? (int)threadIdx.x / cpt : 0;
  const int h0 = ((int)threadIdx.x - tl * cpt) * EPU;
  const int hStep = tpb > 1 ? H : (int)blockDim.x * EPU;
  const int nSlot = K + nSh;
  for (int t = blockIdx.x * tpb + tl; t < S && tl < tpb;
       t += gridDim.x * tpb) {
    bool kp[K];
#pragma unroll
    for (int j = 0; j < K; ++j) kp[j] = kept[(size_t)t * K + j] != 0;
    const T* slots = cbuf + (size_t)t * nSlot * H;
    for (int h = h0; h < H; h += hStep) {
      float acc[EPU];
#pragma unroll
      for (int q = 0; q < EPU; ++q) acc[q] = 0.0f;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (!kp[j]) continue;
        accSlot16<T>(slots + (size_t)j * H + h, acc);
      }
      for (int s = 0; s < nSh; ++s)
        accSlot16<T>(slots + (size_t)(K + s) * H + h, acc);
      T ov[EPU];
#pragma unroll
      for (int q = 0; q < EPU; ++q) fromF(acc[q], ov[q]);
      *reinterpret_cast<u32x4*>(out + (size_t)t * H + h) =
          *reinterpret_cast<const u32x4*>(ov);
    }
  }
  FM_AUX_STAMP(1, 1);
}

// cast the fp32 combine accumulator into the Element output (k>1 path)
// and RE-ZERO it for the next forward (O32 is zeroed once at initialize;
// keeping it clean here saves a 16 MB memset pass per call)
template <typename T>
__global__ void k_cast_out(float* __restrict__ O32, T* __restrict__ out,
                           size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t j = i; j < n; j += stride) {
    fromF(O32[j], out[j]);
    O32[j] = 0.0f;
  }
}

// combine pre-packed return rows (EP host path): one block per row
template <typename T, bool SCALED>
__global__ void k_combine_rows(const T* __restrict__ rows,
                               const uint32_t* __restrict__ tokenIdx,
                               const float* __restrict__ scale,
                               float* __restrict__ O32, T* __restrict__ moeOut,
                               int H) {
  const int i = blockIdx.x;
  const uint32_t t = tokenIdx[i];
  const float s = SCALED ? scale[i] : 1.0f;
  for (int h = threadIdx.x; h < H; h += blockDim.x) {
    const float v = toF(rows[(size_t)i * H + h]);
    if (SCALED)
      atomicAdd(&O32[(size_t)t * H + h], s * v);
    else
      moeOut[(size_t)t * H + h] = rows[(size_t)i * H + h];
  }
}

// pack the dispatch send buffer: send[e][i][:] = x[tokenIds[e][i]][:]
// for i < min(eC[e], EC); rows past the routed count keep whatever is
// there (they are dropped at the source on combine). This is the
// reference's symmetric-heap cell layout (peer-major expert-slot cells,
// types.cuh:1014-1032) built for a capacity-padded static all_to_all.
template <typename T>
__global__ void k_pack_dispatch(const T* __restrict__ x,
                                const TPS* __restrict__ tokenIds,
                                const uint32_t* __restrict__ eC,
                                T* __restrict__ sendbuf, int H, int EC,
                                int pEC) {
  const int e = blockIdx.y;
  const int i = blockIdx.x;
  const uint32_t r = min(eC[e], (uint32_t)EC);
  if ((uint32_t)i >= r) return;
  const uint32_t tok = tpsTok(tokenIds[(size_t)e * pEC + i].tokenIdx);
  constexpr int EPU = 16 / sizeof(T);  // elements per 16B unit
  const T* src = x + (size_t)tok * H;
  T* dst = sendbuf + ((size_t)e * EC + i) * H;
  for (int h = threadIdx.x * EPU; h < H; h += blockDim.x * EPU) {
    *reinterpret_cast<u32x4*>(dst + h) =
        *reinterpret_cast<const u32x4*>(src + h);
  }
}

// combine the capacity-padded RETURNED buffer at the source: for each
// (e, i < routed), out[token] += gate_out[token, e]/probSum * row
// (k>1; k==1 unscaled overwrite semantics via scale=1 on a zero
// accumulator). All metadata is source-local (tokenIds/eC/gate_out) -
// no host involvement (processor.cuh:44-205 combine semantics).
template <typename T>
__global__ void k_combine_padded(const T* __restrict__ rows,
                                 const TPS* __restrict__ tokenIds,
                                 const uint32_t* __restrict__ eC,
                                 const T* __restrict__ gate_out,
                                 T* __restrict__ cbuf, int H, int EC,
                                 int pEC, int PX, int topk) {
  const int e = blockIdx.y;
  const int i = blockIdx.x;
  const uint32_t r = min(eC[e], (uint32_t)EC);
  if ((uint32_t)i >= r) return;
  const TPS tp = tokenIds[(size_t)e * pEC + i];
  const uint32_t tok = tpsTok(tp.tokenIdx);
  const uint32_t j = tpsJ(tp.tokenIdx);
  const float sc = (topk > 1)
      ? toF(gate_out[(size_t)tok * PX + e]) / tp.probSum
      : 1.0f;
  const T* src = rows + ((size_t)e * EC + i) * H;
  // non-atomic per-(token, j) combine slot (k_cast_combine sums them)
  T* dst = cbuf + ((size_t)tok * topk + j) * H;
  for (int h = threadIdx.x; h < H; h += blockDim.x) {
    fromF(sc * toF(src[h]), dst[h]);
  }
}

// ---------------------------------------------------------------------------
// One-sided P2P dispatch/return over xGMI (the reference's intra-node
// mode: direct stores into peers' symmetric-heap cells + system-scope
// 8-byte signals, os/packet.cuh:214-258 / bootstrap.cuh:442-443
// nvshmem_ptr resolution). Heap cell layout identical to the padded
// all_to_all path ([source, local expert, slot<EC, H]); flags are
// seq-tagged so they never need re-zeroing (seqBit concept,
// types.cuh:1045-1063). Visibility protocol per the CDNA4 guide
// (Guideline 16, system scope for cross-device): payload stores ->
// per-wave vmcnt drain -> one-lane system-scope release fence + asm
// vmcnt drain -> relaxed system-scope flag store; consumer polls
// relaxed, then one system-scope acquire fence.
// ---------------------------------------------------------------------------

// write this rank's routed rows for expert e straight into the OWNER
// rank's recv heap cell [myRank][e%nLx][i]; the last arriving block of
// each expert signals the owner's dispatch flag with `seq`.
template <typename T>
__global__ void k_dispatch_p2p(const T* __restrict__ x,
                               const TPS* __restrict__ tokenIds,
                               const uint32_t* __restrict__ eC,
                               const uint64_t* __restrict__ peerRecv,
                               const uint64_t* __restrict__ peerDispFlags,
                               uint32_t* __restrict__ arrive, int H, int EC,
                               int pEC, int nLx, int myRank,
                               unsigned long long seq) {
  const int e = blockIdx.y;
  const int i = blockIdx.x;
  const uint32_t r = min(eC[e], (uint32_t)EC);
  const uint32_t participants = max(r, 1u);
  if ((uint32_t)i >= participants) return;
  const int owner = e / nLx;
  const int le = e % nLx;
  T* heap = reinterpret_cast<T*>(peerRecv[owner]);
  if ((uint32_t)i < r) {
    const uint32_t tok = tpsTok(tokenIds[(size_t)e * pEC + i].tokenIdx);
    const T* src = x + (size_t)tok * H;
    T* dst = heap + (((size_t)myRank * nLx + le) * EC + i) * H;
    constexpr int EPU = 16 / sizeof(T);
    for (int h = threadIdx.x * EPU; h < H; h += blockDim.x * EPU) {
      *reinterpret_cast<u32x4*>(dst + h) =
          *reinterpret_cast<const u32x4*>(src + h);
    }
  }
  // every wave drains its own stores before the block arrives
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t got = __hip_atomic_fetch_add(
        arrive + e, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (got + 1 == participants) {
      // last arriver publishes to the owner: system release + flag
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      unsigned long long* flag =
          reinterpret_cast<unsigned long long*>(peerDispFlags[owner]) +
          (size_t)myRank * nLx + le;
      __hip_atomic_store(flag, seq, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// wait until every (source, local expert) dispatch flag equals seq.
// On timeout the device error word (host-mapped, zero-copy) is set so
// the host can detect the poisoned exchange without a stream sync:
// fm_dispatch_p2p/fm_return_p2p check it at entry and
// fm_p2p_error_check() checks it definitively after a sync.
__global__ void k_await_flags(const unsigned long long* __restrict__ flags,
                              int n, unsigned long long seq,
                              uint32_t* __restrict__ err, long long maxSpin) {
  bool done = false;
  for (long long spin = 0; !done && spin < maxSpin; ++spin) {
    done = true;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      done &= (__hip_atomic_load(flags + i, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_SYSTEM) >= seq);
    }
    done = __syncthreads_and(done);
    if (!done) __builtin_amdgcn_s_sleep(16);
  }
  if (threadIdx.x == 0 && !done) {
    // bounded spin gave up: poison is preferable to a hang, but the
    // host MUST be able to see it happened
    printf("flashmoe: k_await_flags timeout (seq %llu)\n", seq);
    if (err)
      __hip_atomic_store(err, (uint32_t)seq ? (uint32_t)seq : 1u,
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  __syncthreads();
}

// return the FFN results: segment (s, le) rows go back to source rank
// s's return heap at cell [global expert][i]; last block per segment
// signals the source's return flag for that global expert.
template <typename T>
__global__ void k_return_p2p(const T* __restrict__ ffn_out,
                             const uint64_t* __restrict__ peerRet,
                             const uint64_t* __restrict__ peerRetFlags,
                             uint32_t* __restrict__ arrive, int H, int EC,
                             int nLx, int myRank,
                             unsigned long long seq) {
  const int seg = blockIdx.y;  // (source rank, local expert)
  const int i = blockIdx.x;
  const int src = seg / nLx;
  const int le = seg % nLx;
  const int ge = myRank * nLx + le;  // global expert id (I am the owner)
  T* ret = reinterpret_cast<T*>(peerRet[src]);
  const T* row = ffn_out + ((size_t)seg * EC + i) * H;
  T* dst = ret + ((size_t)ge * EC + i) * H;
  constexpr int EPU = 16 / sizeof(T);
  for (int h = threadIdx.x * EPU; h < H; h += blockDim.x * EPU) {
    *reinterpret_cast<u32x4*>(dst + h) =
        *reinterpret_cast<const u32x4*>(row + h);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t got = __hip_atomic_fetch_add(
        arrive + seg, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (got + 1 == (uint32_t)EC) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      unsigned long long* flag =
          reinterpret_cast<unsigned long long*>(peerRetFlags[src]) + ge;
      __hip_atomic_store(flag, seq, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// export clipped routing into caller tensors: routed[e] = min(eC, EC),
// out[e][i] = {tokenIdx, probSum-bits} for i < routed (EP host pipeline)
__global__ void k_export_routing(const TPS* __restrict__ tokenIds,
                                 const uint32_t* __restrict__ eC,
                                 uint32_t* __restrict__ routed,
                                 uint32_t* __restrict__ out, int E, int EC,
                                 int pEC) {
  const int e = blockIdx.x;
  const uint32_t r = min(eC[e], (uint32_t)EC);
  if (threadIdx.x == 0) routed[e] = r;
  for (int i = threadIdx.x; i < EC; i += blockDim.x) {
    TPS t = (i < (int)r) ? tokenIds[(size_t)e * pEC + i] : TPS{0u, 0.0f};
    out[((size_t)e * EC + i) * 2] = tpsTok(t.tokenIdx);
    out[((size_t)e * EC + i) * 2 + 1] = __float_as_uint(t.probSum);
  }
}

// MX-scaled MFMA layout probe (test-only): D = block-scaled A[16x128] x
// B[128x16] via one mfma_scale_f32_16x16x128_f8f6f4 (fp8 e4m3 A and B,
// E8M0 scales). Empirically pinned contract (test_mx_mfma_layout_probe):
// lane l holds A[row=l&15][k=32*(l>>4)..+32] and B[...][col=l&15] as 8
// dwords; the scale byte of lane-group g covers the interleaved chunk
// pair {k: k>>6 == g&1, (k>>4)&1 == g>>1} (so per-contiguous-64 scales
// are supplied as block (g&1)); value 2^(byte-127); C/D as every 16x16.
template <int OPS>
__global__ void k_mx_mfma_probe(const uint8_t* A, const uint8_t* B,
                                const uint8_t* sa, const uint8_t* sb,
                                float* D) {
  const int lane = threadIdx.x & 63;
  const int row = lane & 15;
  const int kb = lane >> 4;  // 32-element K block (assumed data layout)
  i32x8 af, bf;
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    af[d] = *reinterpret_cast<const int*>(&A[row * 128 + kb * 32 + d * 4]);
    bf[d] = *reinterpret_cast<const int*>(&B[row * 128 + kb * 32 + d * 4]);
    // B given transposed: B_t[col][k] with col=lane&15 - same indexing
  }
  f32x4 c{0.f, 0.f, 0.f, 0.f};
  // sa/sb are PER-LANE raw scale i32s (64 each): the GPU layout test
  // sweeps single lanes/bytes to pin the hardware's scale->block map
  const int sav = reinterpret_cast<const int*>(sa)[lane];
  const int sbv = reinterpret_cast<const int*>(sb)[lane];
  c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, bf, c, 0, 0,
                                                       OPS, sav, OPS, sbv);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    D[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = c[r];
}

// MFMA layout probe (test-only): D = A[16x32] x B[32x16] via one
// mfma_f32_16x16x32_bf16, written with the assumed C/D mapping.
__global__ void k_fp8cvt_probe(const uint32_t* in, float* out) {
  const int t = threadIdx.x;  // 32 threads x 8 values
  const bf16x8 v = dequant_fp8x8_bf16(in[t * 2], in[t * 2 + 1]);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[t * 8 + i] = (float)v[i];
}

__global__ void k_mfma_probe(const bf16* A, const bf16* B, float* D) {
  const int lane = threadIdx.x & 63;
  bf16x8 af, bfr;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    af[j] = *reinterpret_cast<const __bf16*>(
        &A[(lane & 15) * 32 + (lane >> 4) * 8 + j]);
    bfr[j] = *reinterpret_cast<const __bf16*>(
        &B[(lane & 15) * 32 + (lane >> 4) * 8 + j]);  // B given as [16 col][32 k]
  }
  f32x4 c{0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr, c, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) D[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = c[r];
}

// ===========================================================================
// Fused persistent forward kernel (the north star's single-launch DMoE,
// reference moe::forward, moe.cuh:77-144): ONE launch whose resident
// blocks walk four job phases -
//   L: gate-logits GEMM tiles (K-split, fp32 atomic accumulate into
//      logits32) with per-tile arrival counters; the LAST arriving block
//      of a tile runs the softmax/top-k/route for that tile inline
//      (gate.cuh:474-720 semantics, fused per VERDICT r01 #4)
//   U: expert up-GEMM tiles (act(x W_up^T + b), token-gather A)
//   D: expert down-GEMM tiles with the combine-slot epilogue
//   C: masked slot reduction into moe_out
// Phase seams are job-done fan-ins + one release per producing block,
// following the CDNA4 guide's Guideline 16 protocol exactly: payload
// plain stores -> every wave s_waitcnt vmcnt(0) -> __syncthreads ->
// lane 0 agent-scope release fence + asm vmcnt drain -> relaxed counter
// add; consumers poll relaxed, then ONE agent acquire + __syncthreads.
// All polled words are zeroed by hipMemsetAsync nodes ahead of the
// launch (replayed first under hipGraph capture). Every spin is bounded
// and a give-up sets the host-mapped error word instead of hanging.
// The grid is sized to exactly the co-resident block count (1 block/CU
// at the 146 KB LDS arena), so the in-kernel waits cannot deadlock.
// ===========================================================================

struct FusedCtl {
  uint32_t routeTilesDone;   // fan-in: tiles fully routed
  uint32_t upJobsDone;       // fan-in: up-GEMM jobs completed
  uint32_t dnJobsDone;       // fan-in: down-GEMM jobs completed
  uint32_t pad0;
  unsigned long long clk[6]; // atomicMax phase-end wall clocks:
                             // 0 entry, 1 route done, 2 up, 3 down, 4 end
  // followed in the same allocation by tileArrive[nTiles]
};

__device__ __forceinline__ void fused_release_arrive(uint32_t* ctr) {
  // producer side of the Guideline 16 hand-off (counter form)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    // restate the post-wbl2 drain where the compiler would drop it
    // (guide Guideline 16 pitfall 12)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
  }
}

__device__ __forceinline__ void fused_wait(const uint32_t* ctr,
                                           uint32_t target,
                                           uint32_t* errWord,
                                           long long bound,
                                           bool noAcq = false) {
  if (threadIdx.x == 0) {
    long long spins = 0;
    while (__hip_atomic_load(ctr, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(64);
      if (++spins > bound) {
        // give up: poisoned output, host sees the error word
        if (errWord)
          __hip_atomic_store(errWord, 2u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_SYSTEM);
        break;
      }
    }
    if (!noAcq) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
}

struct FusedMeta {
  FusedCtl* ctl;
  uint32_t* tileArrive;      // [nTiles] logits-job arrivals per tile
  uint32_t* upRowDone;       // [E, upMT] completed up n-tiles per row-tile
  int upBM, upRowTarget;     // up tile rows / n-tiles per complete row
  uint32_t* eCf;             // per-expert routed counts (g.eC)
  float* logits32;
  void* gate_out;
  TPS* tokenIds;
  const void* cbuf;          // combine slots [S, k, H] Element
  uint8_t* kept;
  void* moe_out;
  float* gML;                // training aux (null in inference)
  float* gMeC;
  uint32_t* errWord;         // host-mapped (system scope)
  int S, H, E, PX, EC, pEC, topk, training;
  int nTiles;                // S / 128
  int lgKS, lgNT, lgJobs;    // logits K-split, N tiles, total jobs
  int upGeom, upMT, upNT, upJobs;
  int dnGeom, dnMT, dnNT, dnJobs;
  int cbTB, cbJobs;          // combine token-block size / jobs
  int debugBits;             // FM_FUSED_DEBUG bit0: skip per-job drains
                             // (publish once at walk end), bit1: skip
                             // acquire fences. MEASUREMENT ONLY - both
                             // break the visibility protocol; never set
                             // outside an A/B pricing run.
  int nBlocks;
  int ctlOff;                // LDS offset of the 16-B control slice
  long long spinBound;
};

// softmax / top-k / ordered placement for one 128-token tile inside the
// fused kernel: thin wrapper over route_tile_core (shared with the
// classic k_gate_route)
template <typename T, int K>
__device__ __forceinline__ void route_tile(char* smem, const FusedMeta& f,
                                           int tile) {
  route_tile_core<T, K>(smem, f.logits32, reinterpret_cast<T*>(f.gate_out),
                        f.tokenIds, f.eCf, f.kept, f.gML, f.gMeC, f.S, f.E,
                        f.PX, f.EC, f.pEC, tile * 128);
}

// masked slot reduction (k_cast_combine semantics) over a token block
template <typename T, int K>
__device__ __forceinline__ void combine_tokens(const FusedMeta& f, int t0,
                                               int t1) {
  constexpr int EPU = 16 / sizeof(T);
  const T* cbuf = reinterpret_cast<const T*>(f.cbuf);
  T* out = reinterpret_cast<T*>(f.moe_out);
  const int H = f.H;
  // flat (token, h-unit) sweep: keeps all 512 threads busy even when
  // H/EPU < 512 (the per-token h loop left 3/4 of the block idle)
  const int units = H / EPU;
  const int total = (t1 - t0) * units;
  for (int u = threadIdx.x; u < total; u += 512) {
    const int t = t0 + u / units;
    const int h = (u % units) * EPU;
    {
      float acc[EPU];
#pragma unroll
      for (int q = 0; q < EPU; ++q) acc[q] = 0.0f;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (f.kept[(size_t)t * K + j] == 0) continue;
        const u32x4 v = *reinterpret_cast<const u32x4*>(
            cbuf + ((size_t)t * K + j) * H + h);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const uint32_t vw = v[w];
          if constexpr (__is_same(T, bf16)) {
            const float2 fv = __bfloat1622float2(
                *reinterpret_cast<const __hip_bfloat162*>(&vw));
            acc[2 * w] += fv.x;
            acc[2 * w + 1] += fv.y;
          } else if constexpr (__is_same(T, fp16)) {
            const float2 fv = __half22float2(
                *reinterpret_cast<const __half2*>(&vw));
            acc[2 * w] += fv.x;
            acc[2 * w + 1] += fv.y;
          } else {
            acc[w] += __uint_as_float(vw);
          }
        }
      }
      T ov[EPU];
#pragma unroll
      for (int q = 0; q < EPU; ++q) fromF(acc[q], ov[q]);
      *reinterpret_cast<u32x4*>(out + (size_t)t * H + h) =
          *reinterpret_cast<const u32x4*>(ov);
    }
  }
}

// static XCD-swizzled walk over one GEMM phase's (e, mT, nT) jobs
// (identical swizzle to the classic persistent grid)
template <typename ET, int PHASE, int BN, int BM, typename WET, int STAGES,
          int CK = 0, int CN = 0>
__device__ __forceinline__ void gemm_phase_walk(const GemmArgs& a, char* smem,
                                                int mT, int nT, int nJobs,
                                                int nBlocks, int act,
                                                int hasBias,
                                                uint32_t* doneCtr,
                                                uint32_t* rowDone,
                                                int debugBits) {
  const int qx = nJobs / 8, rx = nJobs % 8;
  int par = 0;  // gemm_job_body metadata copy; flips after a job that ran
  for (int jl = blockIdx.x; jl < nJobs; jl += nBlocks) {
    const int xcd = jl % 8, pos = jl / 8;
    const int swz =
        (xcd < rx ? xcd * (qx + 1) : rx * (qx + 1) + (xcd - rx) * qx) + pos;
    const int e = swz / (mT * nT);
    const int rem = swz % (mT * nT);
    const bool ran =
        gemm_job_body<ET, PHASE, BN, BM, WET, STAGES, CK, CN, true>(
            a, smem, e, 0, (rem % mT) * BM, (rem / mT) * BN, act,
            hasBias != 0, par);
    par ^= ran ? 1 : 0;
    // job-count arrival: the epilogue's sc1 write-through stores need
    // only a per-wave drain before the relaxed arrival (Guideline 16
    // R1) - no cache-flushing release fence per block. Row arrivals
    // (rowDone) progressively unlock the down phase's dependent tiles.
    if (ran && !(debugBits & 1)) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      __hip_atomic_fetch_add(doneCtr, 1u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
      if (ran && rowDone)
        __hip_atomic_fetch_add(rowDone + (size_t)e * mT + (rem % mT), 1u,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// down-phase walk: each job first waits (bounded) for the up row-tiles
// covering its A rows, takes ONE agent acquire, then runs - the down
// phase overlaps the up phase's tail instead of waiting for all of it
template <typename ET, int BN, int BM, typename WET, int STAGES,
          int CK = 0, int CN = 0>
__device__ __forceinline__ void gemm_phase_walk_dn(
    const GemmArgs& a, const FusedMeta& f, char* smem, int mT, int nT,
    int nJobs, int nBlocks, int hasBias, uint32_t* doneCtr) {
  const int qx = nJobs / 8, rx = nJobs % 8;
  int par = 0;  // as in gemm_phase_walk
  for (int jl = blockIdx.x; jl < nJobs; jl += nBlocks) {
    const int xcd = jl % 8, pos = jl / 8;
    const int swz =
        (xcd < rx ? xcd * (qx + 1) : rx * (qx + 1) + (xcd - rx) * qx) + pos;
    const int e = swz / (mT * nT);
    const int rem = swz % (mT * nT);
    const int m0 = (rem % mT) * BM;
    // routed counts are final (route fan-in acquired earlier)
    const uint32_t rClip =
        min(__hip_atomic_load(f.eCf + e, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT),
            (uint32_t)a.EC);
    bool ran = false;
    if ((uint32_t)m0 < rClip) {
      if (threadIdx.x == 0) {
        // wait for every up row-tile covering rows [m0, min(m0+BM, rClip))
        const int rowHi =
            ((int)rClip - 1 < m0 + BM - 1) ? (int)rClip - 1 : m0 + BM - 1;
        for (int r = m0 / f.upBM; r <= rowHi / f.upBM; ++r) {
          const uint32_t* ctr = f.upRowDone + (size_t)e * f.upMT + r;
          long long spins = 0;
          while (__hip_atomic_load(ctr, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT) <
                 (uint32_t)f.upRowTarget) {
            __builtin_amdgcn_s_sleep(32);
            if (++spins > f.spinBound) {
              if (f.errWord)
                __hip_atomic_store(f.errWord, 3u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
              break;
            }
          }
        }
        if (!(f.debugBits & 2))
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
      __syncthreads();
      ran = gemm_job_body<ET, 1, BN, BM, WET, STAGES, CK, CN, true>(
          a, smem, e, 0, m0, (rem / mT) * BN, 0, hasBias != 0, par);
      par ^= ran ? 1 : 0;
    }
    if (ran && !(f.debugBits & 1)) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    if (threadIdx.x == 0)
      __hip_atomic_fetch_add(doneCtr, 1u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <typename ET, typename WET, int CH = 0, int CP = 0>
__global__ __launch_bounds__(512, 1) void k_moe_fused(GemmArgs gl, GemmArgs gu,
                                                      GemmArgs gd,
                                                      FusedMeta f) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint32_t* sCtl = reinterpret_cast<uint32_t*>(smem + f.ctlOff);
  const int tid = threadIdx.x;
  if (tid == 0)
    atomicMax(reinterpret_cast<unsigned long long*>(&f.ctl->clk[0]),
              __builtin_amdgcn_s_memrealtime());

  // ---- phase L: gate logits tiles + inline route on last arrival ----
  const int jobsPerTile = f.lgKS * f.lgNT;
  for (int j = blockIdx.x; j < f.lgJobs; j += f.nBlocks) {
    const int t = j % f.nTiles;
    const int rest = j / f.nTiles;
    const int ks = rest % f.lgKS;
    const int nt = rest / f.lgKS;
    // (block barriers follow every logits job: metadata copy 0 is free)
    (void)gemm_job_body<ET, 3, 128, 128, ET, 2, CH, 0>(gl, smem, 0, ks,
                                                        t * 128, nt * 128, 0,
                                                        false, 0);
    // arrive on the tile: the logits writes are fp32 atomicAdds
    // (globally coherent), so only a vmcnt drain orders them before
    // the arrival; no cache release is needed
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0)
      *sCtl = __hip_atomic_fetch_add(f.tileArrive + t, 1u, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const bool last = (*sCtl == (uint32_t)(jobsPerTile - 1));
    __syncthreads();  // everyone read sCtl before the next iteration
    if (last) {
      if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      __syncthreads();
      switch (f.topk) {
        case 1: route_tile<ET, 1>(smem, f, t); break;
        case 2: route_tile<ET, 2>(smem, f, t); break;
        case 3: route_tile<ET, 3>(smem, f, t); break;
        case 4: route_tile<ET, 4>(smem, f, t); break;
        case 5: route_tile<ET, 5>(smem, f, t); break;
        case 6: route_tile<ET, 6>(smem, f, t); break;
        case 7: route_tile<ET, 7>(smem, f, t); break;
        default: route_tile<ET, 8>(smem, f, t); break;
      }
      fused_release_arrive(&f.ctl->routeTilesDone);
    }
  }
  fused_wait(&f.ctl->routeTilesDone, (uint32_t)f.nTiles, f.errWord,
             f.spinBound, (f.debugBits & 2) != 0);
  if (tid == 0)
    atomicMax(reinterpret_cast<unsigned long long*>(&f.ctl->clk[1]),
              __builtin_amdgcn_s_memrealtime());

  // ---- phase U: expert up-GEMM ----
  switch (f.upGeom) {
    case 0:
      gemm_phase_walk<ET, 0, 256, 256, WET, 2, CH, CP>(
          gu, smem, f.upMT, f.upNT, f.upJobs, f.nBlocks, gu.act,
          gu.bias != nullptr, &f.ctl->upJobsDone, f.upRowDone,
          f.debugBits);
      break;
    case 1:
      gemm_phase_walk<ET, 0, 128, 256, WET, 3, CH, CP>(
          gu, smem, f.upMT, f.upNT, f.upJobs, f.nBlocks, gu.act,
          gu.bias != nullptr, &f.ctl->upJobsDone, f.upRowDone,
          f.debugBits);
      break;
    case 3:
      gemm_phase_walk<ET, 0, 256, 128, WET, 3, CH, CP>(
          gu, smem, f.upMT, f.upNT, f.upJobs, f.nBlocks, gu.act,
          gu.bias != nullptr, &f.ctl->upJobsDone, f.upRowDone,
          f.debugBits);
      break;
    default:
      gemm_phase_walk<ET, 0, 128, 128, WET, 2, CH, CP>(
          gu, smem, f.upMT, f.upNT, f.upJobs, f.nBlocks, gu.act,
          gu.bias != nullptr, &f.ctl->upJobsDone, f.upRowDone,
          f.debugBits);
      break;
  }
  // no global up->down seam: each down job waits only for the up
  // row-tiles covering its A rows (gemm_phase_walk_dn); clk[2] marks
  // this block's transition into the down walk
  if (tid == 0)
    atomicMax(reinterpret_cast<unsigned long long*>(&f.ctl->clk[2]),
              __builtin_amdgcn_s_memrealtime());

  // ---- phase D: expert down-GEMM with combine-slot epilogue ----
  switch (f.dnGeom) {
    case 0:
      gemm_phase_walk_dn<ET, 256, 256, WET, 2, CP, CH>(
          gd, f, smem, f.dnMT, f.dnNT, f.dnJobs, f.nBlocks,
          gd.bias != nullptr, &f.ctl->dnJobsDone);
      break;
    case 1:
      gemm_phase_walk_dn<ET, 128, 256, WET, 3, CP, CH>(
          gd, f, smem, f.dnMT, f.dnNT, f.dnJobs, f.nBlocks,
          gd.bias != nullptr, &f.ctl->dnJobsDone);
      break;
    case 3:
      gemm_phase_walk_dn<ET, 256, 128, WET, 3, CP, CH>(
          gd, f, smem, f.dnMT, f.dnNT, f.dnJobs, f.nBlocks,
          gd.bias != nullptr, &f.ctl->dnJobsDone);
      break;
    default:
      gemm_phase_walk_dn<ET, 128, 128, WET, 2, CP, CH>(
          gd, f, smem, f.dnMT, f.dnNT, f.dnJobs, f.nBlocks,
          gd.bias != nullptr, &f.ctl->dnJobsDone);
      break;
  }
  fused_wait(&f.ctl->dnJobsDone, (uint32_t)f.dnJobs, f.errWord,
             f.spinBound, (f.debugBits & 2) != 0);
  if (tid == 0)
    atomicMax(reinterpret_cast<unsigned long long*>(&f.ctl->clk[3]),
              __builtin_amdgcn_s_memrealtime());

  // ---- phase C: masked slot reduction ----
  for (int j = blockIdx.x; j < f.cbJobs; j += f.nBlocks) {
    const int t0 = j * f.cbTB;
    const int t1 = min(f.S, t0 + f.cbTB);
    switch (f.topk) {
      case 1: combine_tokens<ET, 1>(f, t0, t1); break;
      case 2: combine_tokens<ET, 2>(f, t0, t1); break;
      case 3: combine_tokens<ET, 3>(f, t0, t1); break;
      case 4: combine_tokens<ET, 4>(f, t0, t1); break;
      case 5: combine_tokens<ET, 5>(f, t0, t1); break;
      case 6: combine_tokens<ET, 6>(f, t0, t1); break;
      case 7: combine_tokens<ET, 7>(f, t0, t1); break;
      default: combine_tokens<ET, 8>(f, t0, t1); break;
    }
  }
  if (tid == 0)
    atomicMax(reinterpret_cast<unsigned long long*>(&f.ctl->clk[4]),
              __builtin_amdgcn_s_memrealtime());
}

// ===========================================================================
// Host side: state, workspace, ABI
// ===========================================================================

static int launch_group_gemm(hipStream_t st, int phase, const struct GemmArgs& a,
                             int M, int nE);

namespace {

struct State {
  fm_config cfg{};
  bool initialized = false;
  int rank = 0, world = 1;
  int S = 0, H = 0, P = 0, E = 0, PX = 0, nLx = 0, EC = 0, pEC = 0;
  size_t esz = 0;
  size_t wesz = 0;  // expert-weight element size (1 for fp8 weights)
  int wMats = 2;    // [P,H] slabs per expert: 2 (up, down), or 3 for gated
                    // experts (hidden_act 2/3: up, down, gating projection)
  bool gated = false;
  // shared experts (num_shared_experts): nSh FFNs applied
  // to every token, run as nV = nSh * ceil(S / min(EC, S)) extra z-slices
  // of the two expert GEMM launches
  int nSh = 0;
  int nV = 0;
  int32_t* sliceExpert = nullptr;  // [E + nV] z -> weight expert (nSh > 0)
  // workspace
  TPS* tokenIds = nullptr;   // [E + nV, pEC]; the nV tail is static
  uint32_t* eC = nullptr;    // [E + nV]; the gates write the first E only
  float* logits32 = nullptr; // [S, E] gate logit accumulator
  float* gML = nullptr;      // [E] training aux: mean gate prob
  float* gMeC = nullptr;     // [E] training aux: routed fraction
  // single-launch gate (k_gate_fused): one allocation, 16-B aligned parts:
  //   tilesDone + pad | tileArrive[S/128] | eCacc[E]   (zero after use)
  //   | gateCw[S] f32 | gateSel[S, k] u16              (hand-off payload)
  uint32_t* gateCtl = nullptr;
  size_t gateArriveOff = 0, gateEcOff = 0, gateCwOff = 0, gateSelOff = 0;
  // one-sided P2P heap (opt-in EP transport)
  char* heap = nullptr;      // local block: recv | ret | dispFlags | retFlags
  size_t heapRecvOff = 0, heapRetOff = 0, heapDFlagOff = 0, heapRFlagOff = 0;
  size_t heapBytes = 0;
  void* peerBase[64] = {};   // opened peer heap bases (self = heap)
  bool peerOpened[64] = {};  // true only for real hipIpcOpenMemHandle maps
  uint64_t* dPeerRecv = nullptr;   // device tables [world]
  uint64_t* dPeerRet = nullptr;
  uint64_t* dPeerDFlag = nullptr;
  uint64_t* dPeerRFlag = nullptr;
  uint32_t* dArrive = nullptr;     // [2*E] dispatch/return arrival counters
  uint32_t* hP2pErr = nullptr;     // host-mapped timeout flag (zero-copy)
  uint32_t* dP2pErr = nullptr;     // device view of hP2pErr
  unsigned long long seq = 0;
  // transparent hipGraph cache for repeated-pointer forwards
  hipGraphExec_t graphExec = nullptr;
  void* graphKey[10] = {};
  void* lastKey[10] = {};
  bool graphValid = false;
  void* xM = nullptr;        // [nLx_alloc, pEC, P] Element
  uint8_t* x8 = nullptr;     // dtype 5: quantized activations [S, H]
  uint8_t* xs = nullptr;     // dtype 5: x block scales [S, H/64]
  uint8_t* xM8 = nullptr;    // dtype 5: quantized intermediates
  uint8_t* xMs = nullptr;    // dtype 5: xM block scales
  float* O32 = nullptr;      // [S, H] (staged-API combine accumulator)
  void* cbuf = nullptr;      // [S, k, H] Element: non-atomic combine slots
  uint8_t* kept = nullptr;   // [S, k] capacity-kept mask (gate-written)
  int nLxAlloc = 0;
  // fused persistent kernel (single-launch forward)
  FusedCtl* fusedCtl = nullptr;   // device: FusedCtl + tileArrive[nTiles]
  size_t fusedCtlBytes = 0;
  uint32_t* hFusedErr = nullptr;  // host-mapped give-up flag (zero-copy)
  uint32_t* dFusedErr = nullptr;
  int nCU = 0;
  int wallClockKHz = 100000;      // s_memrealtime rate (ticks per ms)
  bool lastForwardFused = false;
  bool lastForwardDecodeFfn = false;  // the last forward took k_decode_ffn
  // router variant (fm_set_router); reset with the State
  fm_router_config router{0, 1, 1, 1, 0, 1.0f, nullptr};
  bool routerRV = false;    // any non-default field: the RV gate kernels
  uint32_t routerGen = 0;   // bumped per fm_set_router: part of the graph key
  // per-output-channel fp32 scales of the fp8 expert weights
  // (fm_set_weight_scales): borrowed device tensor
  // [nLx + nSh, P + H (+ P gated)], record = [s_up | s_dn | s_glu]
  const float* wScale = nullptr;
  int wScaleGran = 0;        // 0 none, 1 per output channel
  uint32_t wScaleGen = 0;    // bumped per set call: part of the graph key
};
State g;

// Point a launch at the weight scales of its phase (0 up, 1 down): the
// record of weight expert `firstExpert`, offset to the phase's vector. The
// kernels add we * stride; entry points that pre-select one expert pass its
// id here and a launch whose z-slices all read that record (stride 0).
static void setWeightScaleArgs(GemmArgs& a, int phase, int firstExpert,
                               bool strided) {
  const long long SC = (long long)g.P + g.H + (g.gated ? g.P : 0);
  a.wScale = g.wScale ? g.wScale + (size_t)firstExpert * SC +
                            (phase == 0 ? 0 : g.P)
                      : nullptr;
  a.wScaleStride = strided ? SC : 0;
  a.wScaleGlu = g.P + g.H;  // s_up -> s_glu inside a record (gated up phase)
}

// kernel-side view of g.router
static RouterP routerParams() {
  RouterP rp{};
  rp.bias = g.router.score_bias;
  rp.factor = g.router.routed_scaling_factor;
  rp.scoring = g.router.scoring_func;
  rp.norm = g.router.norm_topk_prob;
  rp.G = g.router.n_group;
  rp.TG = g.router.topk_group;
  rp.gscore = g.router.group_score;
  rp.selLogits = (rp.scoring == 0 && !rp.bias && rp.gscore == 0) ? 1 : 0;
  return rp;
}

thread_local char g_err[512] = "";

void setErr(const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
}

#define FM_HIP_CHECK(expr)                                                   \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) {                                                  \
      snprintf(g_err, sizeof(g_err), "HIP error %s at %s:%d: %s",            \
               hipGetErrorString(_e), __FILE__, __LINE__, #expr);            \
      return FM_ERR_HIP;                                                     \
    }                                                                        \
  } while (0)

// dtype 5: does the MX grouped GEMM pick the 256^2 tile for (M, N)?
// (mirrored by launch_group_gemm's MX branch; the 256-tile up epilogue
// quantizes in-register, making the xM quant pass unnecessary)
static bool mxBigGeom(int M, int N, int nE) {
  return (M >= 256) && (N >= 256) &&
         DIVUP(M, 256) * DIVUP(N, 256) * nE >= (g.nCU > 0 ? g.nCU : 256);
}

// 256-wide-N MX geometry (128x256 default or FM_MX_GEOM=big): the
// epilogue quantizes in-register in both, so the xM quant pass is
// skipped whenever the up GEMM runs a 256-wide tile
static bool mxWideN(int M, int N, int nE) {
  return (N >= 256) &&
         (mxBigGeom(M, N, nE) ||
          DIVUP(M, 128) * DIVUP(N, 256) * nE >= (g.nCU > 0 ? g.nCU : 256));
}

size_t gate_lds_bytes(int E, size_t esz) {
  // mirrors the k_gate arena: logits + A chunk + G chunk
  return 128 * (E + 1) * sizeof(float) + (128 + E) * (64 + 8) * esz;
}

static bool gateFusedEnabled() {
  // FM_GATE_FUSED=0 forces the two-kernel gate; default on. Re-read per
  // call (tests toggle it) and part of the graph key, like FM_FUSED.
  const char* e = getenv("FM_GATE_FUSED");
  return !(e && e[0] == '0');
}

// does launch_gate take the single-launch k_gate_fused?
static bool gateFusedApplies() {
  // (never at a decode size: k_gate_fused has no ragged tile)
  return g.gateCtl && g.S >= 128 && g.esz == 2 && g.E <= 64 &&
         !g.cfg.is_training && gateFusedEnabled();
}

// sub-block token count of k_gate_fused (16 -> 256 threads, S/16 blocks;
// 32 -> 512 threads, S/32 blocks)
constexpr int kGateTB = 16;

template <typename T>
int launch_gate_fused(hipStream_t st, const void* x, const void* gate_w,
                      void* gate_out, int64_t S) {
  char* ws = reinterpret_cast<char*>(g.gateCtl);
  const RouterP rp = routerParams();
#define GATE_FUSED_RV(KK, RVV)                                                \
  hipLaunchKernelGGL((k_gate_fused<T, KK, kGateTB, RVV>),                     \
                     dim3((unsigned)(S / kGateTB)), dim3(kGateTB * 16), 0,    \
                     st, reinterpret_cast<const T*>(x),                       \
                     reinterpret_cast<const T*>(gate_w),                      \
                     reinterpret_cast<T*>(gate_out),                          \
                     reinterpret_cast<uint16_t*>(ws + g.gateSelOff),          \
                     reinterpret_cast<float*>(ws + g.gateCwOff), g.gateCtl,   \
                     reinterpret_cast<uint32_t*>(ws + g.gateArriveOff),       \
                     reinterpret_cast<uint32_t*>(ws + g.gateEcOff),           \
                     g.tokenIds, g.eC, g.kept, g.H, g.E, g.PX, g.EC, g.pEC,   \
                     rp)
#define GATE_FUSED(KK)                                                        \
  do {                                                                        \
    if (g.routerRV) { GATE_FUSED_RV(KK, true); }                              \
    else { GATE_FUSED_RV(KK, false); }                                        \
  } while (0)
  switch (g.cfg.expert_top_k) {
    case 1: GATE_FUSED(1); break;
    case 2: GATE_FUSED(2); break;
    case 3: GATE_FUSED(3); break;
    case 4: GATE_FUSED(4); break;
    case 5: GATE_FUSED(5); break;
    case 6: GATE_FUSED(6); break;
    case 7: GATE_FUSED(7); break;
    case 8: GATE_FUSED(8); break;
    default: setErr("unsupported expert_top_k (1..8)"); return FM_ERR_UNSUPPORTED;
  }
#undef GATE_FUSED
#undef GATE_FUSED_RV
  FM_HIP_CHECK(hipGetLastError());
  return FM_OK;
}

int launch_gate(hipStream_t st, const void* x, const void* gate_w,
                void* gate_out, int64_t S) {
  // bf16/fp16, E <= 64, inference: one deterministic launch
  if (gateFusedApplies())
    return g.cfg.dtype == 3
               ? launch_gate_fused<fp16>(st, x, gate_w, gate_out, S)
               : launch_gate_fused<bf16>(st, x, gate_w, gate_out, S);
  // split gate: logits GEMM parallelised over (token tile, H chunk),
  // then per-tile softmax/top-k/route (see k_gate_logits/k_gate_route)
  // a decode-sized forward (S < 128) is one ragged tile:
  // the TAIL instantiations mask its rows >= S
  const int tiles = (int)DIVUP(S, 128);
  const bool tail = S < 128;
  int chunksWanted = DIVUP(512, tiles);
  int Hc = DIVUP(DIVUP(g.H, chunksWanted), 64) * 64;
  const int chunks = DIVUP(g.H, Hc);
  const int eChunks = DIVUP(g.E, 128);
  const int Ec = g.E < 128 ? g.E : 128;
  const bool mfmaLogits = (g.esz == 2);  // bf16/fp16: MFMA logits GEMM
  const size_t ldsL = gate_lds_bytes(Ec, g.esz);
  // route arena: TT = 64-token half-passes at E > 256 (route_tile_core)
  const int rTT = (g.E > 256) ? 64 : 128;
  // (RV: + the LDS bias copy and the per-token group scores)
  const size_t ldsR = (size_t)rTT * (g.E + 1) * sizeof(float) +
                      rTT * 8 * 2 * sizeof(uint16_t) + g.E * sizeof(uint32_t) +
                      3 * rTT * sizeof(float) + 64 +
                      (g.routerRV ? (size_t)(g.E + rTT * kMaxGroups) *
                                        sizeof(float)
                                  : 0);
  const RouterP rp = routerParams();
  float* gMLp = g.cfg.is_training ? g.gML : nullptr;
  float* gMeCp = g.cfg.is_training ? g.gMeC : nullptr;
  if (g.cfg.is_training)
    FM_HIP_CHECK(hipMemsetAsync(g.gML, 0, 2 * (size_t)g.E * sizeof(float), st));
#define GATE_LOGITS_T(T, TL)                                                  \
  do {                                                                        \
    if (ldsL > 64 * 1024)                                                     \
      (void)hipFuncSetAttribute(                                              \
          reinterpret_cast<const void*>(&k_gate_logits<T, TL>),               \
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsL);             \
    hipLaunchKernelGGL((k_gate_logits<T, TL>), dim3(tiles, chunks, eChunks),  \
                       dim3(256), ldsL, st, reinterpret_cast<const T*>(x),    \
                       reinterpret_cast<const T*>(gate_w), g.logits32, g.eC,  \
                       (int)S, g.H, g.E, Hc);                                 \
  } while (0)
#define GATE_LOGITS(T) GATE_LOGITS_T(T, false)
#define GATE_ROUTE_RV(T, KK, RVV, TL)                                         \
  do {                                                                        \
    if (ldsR > 64 * 1024)                                                     \
      (void)hipFuncSetAttribute(                                                    \
          reinterpret_cast<const void*>(&k_gate_route<T, KK, RVV, TL>),       \
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsR);             \
    hipLaunchKernelGGL((k_gate_route<T, KK, RVV, TL>), dim3(tiles),           \
                       dim3(512), ldsR, st, g.logits32,                       \
                       reinterpret_cast<T*>(gate_out), g.tokenIds, g.eC,      \
                       (int)S, g.E, g.PX, g.EC, g.pEC, gMLp, gMeCp, g.kept,   \
                       rp);                                                   \
  } while (0)
#define GATE_ROUTE(T, KK)                                                     \
  do {                                                                        \
    if (tail) {                                                               \
      if (g.routerRV) { GATE_ROUTE_RV(T, KK, true, true); }                   \
      else { GATE_ROUTE_RV(T, KK, false, true); }                             \
    } else if (g.routerRV) { GATE_ROUTE_RV(T, KK, true, false); }             \
    else { GATE_ROUTE_RV(T, KK, false, false); }                              \
  } while (0)
#define GATE_K(T)                                                             \
  switch (g.cfg.expert_top_k) {                                               \
    case 1: GATE_ROUTE(T, 1); break;                                          \
    case 2: GATE_ROUTE(T, 2); break;                                          \
    case 3: GATE_ROUTE(T, 3); break;                                          \
    case 4: GATE_ROUTE(T, 4); break;                                          \
    case 5: GATE_ROUTE(T, 5); break;                                          \
    case 6: GATE_ROUTE(T, 6); break;                                          \
    case 7: GATE_ROUTE(T, 7); break;                                          \
    case 8: GATE_ROUTE(T, 8); break;                                          \
    default: setErr("unsupported expert_top_k (1..8)"); return FM_ERR_UNSUPPORTED; \
  }
  if (mfmaLogits) {
    GemmArgs ga{};
    ga.A = x;
    ga.B = gate_w;
    ga.out = g.logits32;
    ga.tokenIds = nullptr;
    ga.eC = g.eC;      // PHASE 3 zeroes it (block 0) for the route kernel
    ga.EC = g.E;
    ga.K = g.H;
    ga.N = g.E;
    ga.nRows = (int)S;
    ga.H = g.H;
    ga.splitK = 1;
    int rc = launch_group_gemm(st, 3, ga, (int)S, 1);
    if (rc != FM_OK) return rc;
  }
  if (g.cfg.dtype == 2 || g.cfg.dtype == 4 || g.cfg.dtype == 5) {
    if (!mfmaLogits) GATE_LOGITS(bf16);
    GATE_K(bf16)
  } else if (g.cfg.dtype == 3) {
    if (!mfmaLogits) GATE_LOGITS(fp16);
    GATE_K(fp16)
  } else {
    if (tail) GATE_LOGITS_T(float, true);
    else GATE_LOGITS(float);
    GATE_K(float)
  }
#undef GATE_K
#undef GATE_ROUTE
#undef GATE_ROUTE_RV
#undef GATE_LOGITS
#undef GATE_LOGITS_T
  FM_HIP_CHECK(hipGetLastError());
  return FM_OK;
}

// ---------------------------------------------------------------------------
// Fused single-launch forward: geometry selection + launch (device side
// above, k_moe_fused). Returns FM_FALLBACK when the fused kernel cannot
// run this shape (classic multi-kernel path takes over).
// ---------------------------------------------------------------------------

static const int FM_FALLBACK = 1000;  // internal sentinel, never ABI-visible

static bool fusedEnabled() {
  // FM_FUSED=1 forces the single-launch kernel, FM_FUSED=0 forces the
  // classic multi-kernel path. Default: fused where it measures faster
  // (deep-K shapes where the classic down-GEMM cannot run its
  // 2-blocks/CU 128^2 mode, P > 8192: cfg4-shape +3%); classic
  // otherwise (cfg2/3/5 measured faster multi-kernel this round -
  // profiles/r02; the fused kernel remains the FM_FUSED=1 path under
  // active optimization).
  // re-read per call: tests toggle it to force fused-path coverage
  const char* e = getenv("FM_FUSED");
  if (e) return e[0] != '0';
  return g.P > 8192;
}

static long long fusedSpinBound() {
  static const long long b = [] {
    const char* e = getenv("FM_FUSED_SPIN_LOG2");
    const int lg = e ? atoi(e) : 24;
    return 1ll << (lg < 4 ? 4 : (lg > 40 ? 40 : lg));
  }();
  return b;
}

// ctl-embedded eC mirror (the fused kernel's routed counts; g.eC is
// untouched by the fused path)
static uint32_t* fusedECPtr() {
  return reinterpret_cast<uint32_t*>(g.fusedCtl + 1) + (g.S / 128) +
         (size_t)g.E * (g.pEC / 128);
}

static int fusedPoisonCheck() {
  if (g.hFusedErr &&
      *reinterpret_cast<volatile uint32_t*>(g.hFusedErr)) {
    *g.hFusedErr = 0;  // ack so the caller may retry
    setErr("fused forward gave up on an in-kernel wait (output poisoned)");
    return FM_ERR_HIP;
  }
  return FM_OK;
}

// host mirror of gemm_lds_bytes<> for the dynamic arena
static int gemmLdsBytesRT(int BM, int BN, int BEZ, int stages) {
  const int SE = (stages == 3 && 3 * BM * 64 * 2 + 3 * BN * 64 * BEZ +
                                      gemm_meta_bytes(BM) > 160 * 1024)
                     ? 2 : stages;
  return SE * BM * 64 * 2 + SE * BN * 64 * BEZ + gemm_meta_bytes(BM);
}

static void fusedGeoDims(int gm, int& bm, int& bn, int& stages) {
  bm = (gm == 0 || gm == 1) ? 256 : 128;
  bn = (gm == 0 || gm == 3) ? 256 : 128;
  stages = (gm == 1 || gm == 3) ? 3 : 2;
}

struct FusedGeo { int geom, mt, nt, jobs; };

// pick the largest tile that still fills the resident grid (mirrors the
// classic mode selection, DESIGN.md par.3, restricted to 1 block/CU)
static FusedGeo fusedPickGeo(int M, int N, int E, int nBlocks,
                             const int* order, int nOrder, int forceGeom) {
  FusedGeo last{};
  for (int i = 0; i < nOrder; ++i) {
    const int gm = order[i];
    int bm, bn, st;
    fusedGeoDims(gm, bm, bn, st);
    if (forceGeom >= 0 && gm != forceGeom) continue;
    if (M < bm && bm > 128) continue;  // do not waste >half the M rows
    const int mt = DIVUP(M, bm), nt = DIVUP(N, bn);
    last = FusedGeo{gm, mt, nt, mt * nt * E};
    if (forceGeom >= 0) return last;
    if (N < bn && bn > 128) continue;  // half-empty B tiles: next option
    if (last.jobs >= nBlocks) return last;
  }
  const int mt = DIVUP(M, 128), nt = DIVUP(N, 128);
  return FusedGeo{4, mt, nt, mt * nt * E};
}

// co-resident blocks/CU for the fused kernel at a given arena size
// (0 = cannot run). The grid is sized to exactly occ x nCU so every
// block is resident and the in-kernel fan-in waits cannot deadlock.
template <typename ET, typename WET, int CH, int CP>
static int fusedOccT(int arena) {
  static int maxDyn = -1;
  if (maxDyn < 0) {
    maxDyn = (hipFuncSetAttribute(
                  reinterpret_cast<const void*>(&k_moe_fused<ET, WET, CH, CP>),
                  hipFuncAttributeMaxDynamicSharedMemorySize,
                  160 * 1024) == hipSuccess)
                 ? 160 * 1024 : 64 * 1024;
  }
  if (arena > maxDyn) return 0;
  static int occArena = -1, occVal = 0;
  if (occArena != arena) {
    occVal = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &occVal, k_moe_fused<ET, WET, CH, CP>, 512, arena) != hipSuccess)
      occVal = 0;
    occArena = arena;
  }
  return occVal;
}

template <typename ET, typename WET>
static int launchFusedT(hipStream_t st, const GemmArgs& gl,
                        const GemmArgs& gu, const GemmArgs& gd,
                        const FusedMeta& f, int arena, int nBlocks) {
  // BASELINE shape dictionary: compile-time (H, P) fold the tile loop's
  // address math and trip counts (the reference freezes these in its
  // compile-time config contract too); generic fallback otherwise
#define FM_LAUNCH_SHAPE(HH, PP)                                                 do {                                                                            hipLaunchKernelGGL((k_moe_fused<ET, WET, HH, PP>), dim3(nBlocks),                                dim3(512), arena, st, gl, gu, gd, f);                      FM_HIP_CHECK(hipGetLastError());                                              return FM_OK;                                                               } while (0)
  if (g.H == 1024 && g.P == 4096) FM_LAUNCH_SHAPE(1024, 4096);
  if (g.H == 2048 && g.P == 8192) FM_LAUNCH_SHAPE(2048, 8192);
  if (g.H == 4096 && g.P == 14336) FM_LAUNCH_SHAPE(4096, 14336);
  FM_LAUNCH_SHAPE(0, 0);
#undef FM_LAUNCH_SHAPE
}

template <typename ET, typename WET>
static int fusedOccShape(int arena) {
  if (g.H == 1024 && g.P == 4096) return fusedOccT<ET, WET, 1024, 4096>(arena);
  if (g.H == 2048 && g.P == 8192) return fusedOccT<ET, WET, 2048, 8192>(arena);
  if (g.H == 4096 && g.P == 14336)
    return fusedOccT<ET, WET, 4096, 14336>(arena);
  return fusedOccT<ET, WET, 0, 0>(arena);
}

static int fusedOcc(int arena) {
  if (g.cfg.dtype == 3) return fusedOccShape<fp16, fp16>(arena);
  if (g.cfg.dtype == 4) return fusedOccShape<bf16, fp8e4m3>(arena);
  return fusedOccShape<bf16, bf16>(arena);
}

template <typename ET, typename WET>
static int launchFused(hipStream_t st, const GemmArgs& gl,
                       const GemmArgs& gu, const GemmArgs& gd,
                       const FusedMeta& f, int arena, int nBlocks) {
  return launchFusedT<ET, WET>(st, gl, gu, gd, f, arena, nBlocks);
}

static int moe_forward_fused(hipStream_t st, const void* x, const void* gate_w,
                             const void* expert_w, const void* b_up,
                             const void* b_dn, void* gate_out,
                             void* moe_out) {
  if (!g.fusedCtl || g.nCU <= 0) return FM_FALLBACK;
  int nBlocks = g.nCU;  // refined to occ x nCU once the arena is known
  const int K = g.cfg.expert_top_k;
  const int BEZ = (int)g.wesz;

  // logits jobs: 128x128 K-split tiles, enough to fill the grid
  const int nTiles = g.S / 128;
  const int lgNT = DIVUP(g.PX, 128);
  int lgKS = 1;
  while (nTiles * lgNT * lgKS < nBlocks && lgKS < 8 &&
         (g.H / 64) % (lgKS * 2) == 0)
    lgKS *= 2;
  const int lgJobs = nTiles * lgNT * lgKS;

  static const int forceUp = [] {
    const char* e = getenv("FM_FUSED_UP");
    return e ? atoi(e) : -1;
  }();
  static const int forceDn = [] {
    const char* e = getenv("FM_FUSED_DN");
    return e ? atoi(e) : -1;
  }();
  const int upOrder[3] = {0, 3, 4};
  const int dnOrder[3] = {1, 3, 4};
  const FusedGeo up = fusedPickGeo(g.pEC, g.P, g.E, nBlocks, upOrder, 3,
                                   forceUp);
  const FusedGeo dn = fusedPickGeo(g.pEC, g.H, g.E, nBlocks, dnOrder, 3,
                                   forceDn);

  // LDS arena: max of every tile body used plus the route scratch,
  // plus the 16-B control slice at the tail
  int bm, bn, stg;
  int arena = gemmLdsBytesRT(128, 128, (int)g.esz, 2);  // logits tile
  fusedGeoDims(up.geom, bm, bn, stg);
  arena = std::max(arena, gemmLdsBytesRT(bm, bn, BEZ, stg));
  fusedGeoDims(dn.geom, bm, bn, stg);
  arena = std::max(arena, gemmLdsBytesRT(bm, bn, BEZ, stg));
  const int rTT = (g.E > 256) ? 64 : 128;  // route half-passes at big E
  const int routeBytes = rTT * (g.E + 1) * 4 + rTT * K * 2 +
                         (rTT * K + 2) * 2 + g.E * 4 + 3 * rTT * 4;
  arena = std::max(arena, routeBytes);
  arena = (arena + 15) / 16 * 16 + 16;
  if (arena > 160 * 1024) return FM_FALLBACK;
  const int occ = fusedOcc(arena);
  if (occ < 1) return FM_FALLBACK;
  nBlocks = std::min(occ, 2) * g.nCU;  // all blocks co-resident

  GemmArgs gl{}, gu{}, gd{};
  FusedMeta f{};
  gl.A = x;
  gl.B = gate_w;
  gl.out = g.logits32;
  gl.K = g.H;
  gl.N = g.E;
  gl.nRows = g.S;
  gl.H = g.H;
  gl.splitK = lgKS;
  // always atomic: the route runs in a DIFFERENT block than the logits
  // tiles, and atomics are globally coherent without a release fence
  gl.atomicLogits = 1;

  gu.A = x;
  gu.B = expert_w;
  gu.bias = b_up;
  gu.out = g.xM;
  gu.gate_out = gate_out;
  gu.tokenIds = g.tokenIds;
  gu.eC = nullptr;  // set to the ctl-embedded eC mirror below
  gu.strideAExpert = 0;
  gu.strideBExpert = (long long)g.wMats * g.P * g.H;
  gu.strideOExpert = (long long)g.pEC * g.P;
  gu.K = g.H;
  gu.N = g.P;
  gu.EC = g.EC;
  gu.pEC = g.pEC;
  gu.PX = g.PX;
  gu.topk = K;
  gu.act = g.cfg.hidden_act;
  gu.H = g.H;
  gu.splitK = 1;
  static const int dbg = [] {
    const char* e = getenv("FM_FUSED_DEBUG");
    return e ? atoi(e) : 0;
  }();
  gu.sc1Out = (dbg & 4) ? 0 : 1;  // xM consumed by down-GEMM blocks

  gd = gu;
  gd.A = g.xM;
  gd.B = reinterpret_cast<const char*>(expert_w) +
           (size_t)g.P * g.H * g.wesz;
  gd.bias = b_dn;
  gd.out = nullptr;
  gd.O32 = reinterpret_cast<float*>(g.cbuf);
  gd.moe_out = moe_out;
  gd.strideAExpert = (long long)g.pEC * g.P;
  gd.K = g.P;
  gd.N = g.H;
  gd.act = 0;
  gd.slotAlways = 1;

  f.ctl = g.fusedCtl;
  f.tileArrive = reinterpret_cast<uint32_t*>(g.fusedCtl + 1);
  f.upRowDone = f.tileArrive + nTiles;
  fusedGeoDims(up.geom, bm, bn, stg);
  f.upBM = bm;
  f.upRowTarget = up.nt;
  f.eCf = fusedECPtr();  // ctl-embedded (one memset covers it)
  f.logits32 = g.logits32;
  f.gate_out = gate_out;
  f.tokenIds = g.tokenIds;
  f.cbuf = g.cbuf;
  f.kept = g.kept;
  f.moe_out = moe_out;
  f.gML = g.cfg.is_training ? g.gML : nullptr;
  f.gMeC = g.cfg.is_training ? g.gMeC : nullptr;
  f.errWord = g.dFusedErr;
  f.S = g.S;
  f.H = g.H;
  f.E = g.E;
  f.PX = g.PX;
  f.EC = g.EC;
  f.pEC = g.pEC;
  f.topk = K;
  f.training = g.cfg.is_training;
  f.nTiles = nTiles;
  f.lgKS = lgKS;
  f.lgNT = lgNT;
  f.lgJobs = lgJobs;
  f.upGeom = up.geom;
  f.upMT = up.mt;
  f.upNT = up.nt;
  f.upJobs = up.jobs;
  f.dnGeom = dn.geom;
  f.dnMT = dn.mt;
  f.dnNT = dn.nt;
  f.dnJobs = dn.jobs;
  f.cbTB = 8;
  f.cbJobs = DIVUP(g.S, 8);
  f.debugBits = dbg;
  f.nBlocks = nBlocks;
  f.ctlOff = arena - 16;
  f.spinBound = fusedSpinBound();

  // per-forward state re-init (Guideline 16: zero every polled word
  // ahead of the launch; these become memset nodes under graph capture)
  gu.eC = f.eCf;
  gd.eC = f.eCf;
  FM_HIP_CHECK(hipMemsetAsync(g.fusedCtl, 0, g.fusedCtlBytes, st));
  if (g.cfg.is_training)
    FM_HIP_CHECK(hipMemsetAsync(g.gML, 0, 2 * (size_t)g.E * sizeof(float), st));

  if (g.cfg.dtype == 3)
    return launchFused<fp16, fp16>(st, gl, gu, gd, f, arena, nBlocks);
  if (g.cfg.dtype == 4)
    return launchFused<bf16, fp8e4m3>(st, gl, gu, gd, f, arena, nBlocks);
  return launchFused<bf16, bf16>(st, gl, gu, gd, f, arena, nBlocks);
}


}  // namespace

extern "C" {

const char* fm_last_error(void) { return g_err; }
int fm_built_for_gfx950(void) { return 1; }

int fm_initialize(const fm_config* cfg, int rank, int world_size) {
  if (g.initialized) { setErr("already initialized"); return FM_ERR_STATE; }
  if (!cfg) { setErr("null config"); return FM_ERR_STATE; }
  g.router = State{}.router;  // a fresh config starts from the default router
  g.routerRV = false;
  g.wScale = nullptr;  // and without weight scales
  g.wScaleGran = 0;
  g.cfg = *cfg;
  g.rank = rank;
  g.world = world_size;
  g.S = cfg->sequence_len * cfg->mini_batch;
  g.H = cfg->hidden_size;
  g.P = cfg->intermediate_size;
  g.E = cfg->num_experts;
  g.PX = DIVUP(g.E, 64) * 64;
  if (cfg->num_experts % world_size != 0) {
    setErr("num_experts must divide by world_size (uniform EP split)");
    return FM_ERR_SHAPE;
  }
  g.nLx = g.E / world_size;
  const int base = cfg->drop_tokens ? DIVUP(g.S, g.E) : g.S;
  g.EC = base * cfg->capacity_factor * cfg->expert_top_k;
  g.pEC = DIVUP(g.EC, 128) * 128;
  switch (cfg->dtype) {
    case 0: case 1: g.esz = 4; break;
    case 2: case 3: g.esz = 2; break;
    case 4: g.esz = 2; break;  // fp8e4m3 expert weights, bf16 activations
    case 5: g.esz = 2; break;  // MX: fp8 weights + runtime-quantized
                               // fp8 activations on the scaled MFMA
    default: setErr("unknown dtype");
             return FM_ERR_UNSUPPORTED;
  }
  g.wesz = (cfg->dtype == 4 || cfg->dtype == 5) ? 1 : g.esz;
  if (cfg->hidden_act < 0 || cfg->hidden_act > 3) {
    setErr("hidden_act must be 0 (relu), 1 (gelu), 2 (swiglu) or 3 (geglu)");
    return FM_ERR_UNSUPPORTED;
  }
  g.gated = cfg->hidden_act >= 2;
  g.wMats = g.gated ? 3 : 2;
  // shared experts: refused loudly where they cannot run (checked ahead of
  // the gated + MX refusal so the message names the key that asked)
  g.nSh = cfg->num_shared_experts;
  if (g.nSh < 0 || g.nSh > 4) {
    setErr("num_shared_experts must be in [0, 4]");
    return FM_ERR_UNSUPPORTED;
  }
  if (cfg->expert_top_k + g.nSh > 16) {
    setErr("expert_top_k + num_shared_experts must be <= 16 (the combine "
           "slot index j has four bits)");
    return FM_ERR_UNSUPPORTED;
  }
  if (g.nSh > 0 && cfg->dtype == 5) {
    setErr("num_shared_experts > 0 is not supported with torch_dtype 5 (MX)");
    return FM_ERR_UNSUPPORTED;
  }
  if (g.nSh > 0 && world_size > 1) {
    setErr("num_shared_experts > 0 is not supported with world_size > 1: "
           "replicate the shared experts and run them on the local tokens "
           "with fm_expert_ffn(local_e = nLx + s) (INTEGRATION.md)");
    return FM_ERR_UNSUPPORTED;
  }
  if (g.gated && cfg->dtype == 5) {
    // the MX up epilogue quantizes 64-column blocks in-register; halving
    // the output width there is separate work (open items)
    setErr("gated hidden_act (2/3) is not supported with torch_dtype 5 (MX)");
    return FM_ERR_UNSUPPORTED;
  }
  if (cfg->dtype == 5 && (cfg->hidden_size % 128 || cfg->intermediate_size % 128)) {
    setErr("dtype 5 (MX fp8) requires H, P multiples of 128 (BK=128)");
    return FM_ERR_SHAPE;
  }
  if (g.E > 512) { setErr("E > 512 not supported this round"); return FM_ERR_UNSUPPORTED; }
  if (world_size > 64) {
    // the P2P peer tables (State.peerBase, fm_heap_connect locals) are
    // sized for 64 ranks - a full 8-node envelope; reject beyond it
    setErr("world_size > 64 not supported");
    return FM_ERR_UNSUPPORTED;
  }
  if (g.S < 1 || (g.S >= 128 && g.S % 128)) {
    // the gate tiles tokens in blocks of 128 (launch_gate); the one ragged
    // tile it masks is the decode-sized forward, S < 128 (DESIGN.md
    // par.5k). A ragged tail behind full tiles is rejected.
    snprintf(g_err, sizeof(g_err),
             "S = sequence_len * mini_batch = %d must be in [1, 127] or a "
             "positive multiple of 128", g.S);
    return FM_ERR_SHAPE;
  }
  if (g.S < 128) {
    // decode-sized forwards: inference on one rank, never MX
    const char* key = cfg->dtype == 5 ? "torch_dtype 5 (MX)"
                      : cfg->is_training ? "is_training 1"
                      : world_size > 1 ? "world_size > 1" : nullptr;
    if (key) {
      snprintf(g_err, sizeof(g_err),
               "%s is not supported with S = sequence_len * mini_batch = %d "
               "< 128 (decode-sized forwards)", key, g.S);
      return FM_ERR_UNSUPPORTED;
    }
  }
  if (cfg->expert_top_k < 1 || cfg->expert_top_k > 8 ||
      cfg->expert_top_k > g.E) {
    setErr("expert_top_k must be in [1, min(E, 8)]");
    return FM_ERR_UNSUPPORTED;
  }
  if (g.H % 64 || g.P % 64) { setErr("H and P must be multiples of 64"); return FM_ERR_SHAPE; }
  // (bf16/fp16 tiles handle H, P % 64 via the B-row clamp and col < N
  // epilogue guards - the round-1 %128 restriction is lifted, matching
  // the schema's contract; covered by the H=192/P=320 parity cases)
  // workspace: tokenIds/eC global-E; xM sized for the worst consumer
  // (single-rank path: E experts; EP path: world*EC rows per local expert)
  g.nLxAlloc = (world_size == 1) ? g.E
                                 : g.nLx * DIVUP(world_size * g.EC, g.pEC);
  // shared experts: each runs over ALL S tokens as ceil(S / C) virtual
  // z-slices of C = min(EC, S) rows, so a slice has the geometry of a
  // routed expert (rows <= EC <= pEC) and the launches need no new case
  const int shC = std::min(g.EC, g.S);
  const int shSlices = DIVUP(g.S, shC);
  g.nV = g.nSh * shSlices;
  g.nLxAlloc += g.nV;  // xM: one [pEC, P] slice per virtual slice (world 1)
  const int nZ = g.E + g.nV;
  FM_HIP_CHECK(hipMalloc(&g.tokenIds, (size_t)nZ * g.pEC * sizeof(TPS)));
  // what the gate kernels index by 128-row tile is sized in whole tiles
  // (S < 128 is one ragged tile; its rows >= S stay untouched)
  const size_t sTile = (size_t)DIVUP(g.S, 128) * 128;
  FM_HIP_CHECK(hipMalloc(&g.logits32, sTile * g.E * sizeof(float)));
  FM_HIP_CHECK(hipMemset(g.logits32, 0, sTile * g.E * sizeof(float)));
  FM_HIP_CHECK(hipMalloc(&g.gML, 2 * (size_t)g.E * sizeof(float)));
  g.gMeC = g.gML + g.E;
  FM_HIP_CHECK(hipMalloc(&g.eC, (size_t)nZ * sizeof(uint32_t)));
  if (g.nV > 0) {
    // The shared slices' routing is the identity and never changes, so
    // the tail [E, E + nV) of tokenIds / eC is written ONCE, here. It
    // survives every forward because both gates touch only the first E
    // entries of eC (k_gate_fused copies E counts; the two-kernel gate
    // zeroes E, in the logits kernel's block 0 or a memset of E words)
    // and only the first E rows of tokenIds. Keep that true.
    // Slice v = s * shSlices + c of shared expert s covers tokens
    // [c * C, min(S, (c + 1) * C)) with j = k + s, probSum 1.
    const int k = g.cfg.expert_top_k;
    std::vector<TPS> hT((size_t)g.nV * g.pEC, TPS{0u, 1.0f});
    std::vector<uint32_t> hC((size_t)g.nV);
    std::vector<int32_t> hMap((size_t)nZ);
    for (int e = 0; e < g.E; ++e) hMap[e] = e;
    for (int s = 0; s < g.nSh; ++s)
      for (int c = 0; c < shSlices; ++c) {
        const int v = s * shSlices + c;
        const int rows = std::min(shC, g.S - c * shC);
        hC[v] = (uint32_t)rows;
        hMap[g.E + v] = g.E + s;
        for (int i = 0; i < rows; ++i)
          hT[(size_t)v * g.pEC + i] =
              TPS{(uint32_t)(c * shC + i) | ((uint32_t)(k + s) << 28), 1.0f};
      }
    FM_HIP_CHECK(hipMemcpy(g.tokenIds + (size_t)g.E * g.pEC, hT.data(),
                           hT.size() * sizeof(TPS), hipMemcpyHostToDevice));
    FM_HIP_CHECK(hipMemcpy(g.eC + g.E, hC.data(),
                           hC.size() * sizeof(uint32_t),
                           hipMemcpyHostToDevice));
    FM_HIP_CHECK(hipMalloc(&g.sliceExpert, (size_t)nZ * sizeof(int32_t)));
    FM_HIP_CHECK(hipMemcpy(g.sliceExpert, hMap.data(),
                           hMap.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice));
  }
  FM_HIP_CHECK(hipMalloc(&g.xM, (size_t)g.nLxAlloc * g.pEC * g.P * g.esz));
  FM_HIP_CHECK(hipMalloc(&g.O32, (size_t)g.S * g.H * sizeof(float)));
  FM_HIP_CHECK(hipMemset(g.O32, 0, (size_t)g.S * g.H * sizeof(float)));
  // combine slots [S, k + nSh, H]; kept stays [S, k] (gate-written, stride k)
  FM_HIP_CHECK(hipMalloc(&g.cbuf, (size_t)g.S * (g.cfg.expert_top_k + g.nSh) *
                                      g.H * g.esz));
  FM_HIP_CHECK(hipMalloc(&g.kept, sTile * g.cfg.expert_top_k));
  if (g.S >= 128 && g.esz == 2 && g.E <= 64 && !g.cfg.is_training) {
    // k_gate_fused workspace; the ticket words are zeroed here once and
    // left zero by every launch (no memset node per forward)
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    g.gateArriveOff = 16;
    g.gateEcOff = g.gateArriveOff + up16((size_t)(g.S / 128) * sizeof(uint32_t));
    g.gateCwOff = g.gateEcOff + up16((size_t)g.E * sizeof(uint32_t));
    g.gateSelOff = g.gateCwOff + up16((size_t)g.S * sizeof(float));
    const size_t bytes =
        g.gateSelOff +
        up16((size_t)g.S * g.cfg.expert_top_k * sizeof(uint16_t));
    FM_HIP_CHECK(hipMalloc(&g.gateCtl, bytes));
    FM_HIP_CHECK(hipMemset(g.gateCtl, 0, bytes));
  }
  if (g.cfg.dtype == 5) {
    // sized for BOTH the single-rank forward (S rows) and the EP
    // segments path (up to nLxAlloc*pEC recv rows)
    const size_t qRows = std::max((size_t)g.S, (size_t)g.nLxAlloc * g.pEC);
    FM_HIP_CHECK(hipMalloc(&g.x8, qRows * g.H));
    FM_HIP_CHECK(hipMalloc(&g.xs, qRows * (g.H / 64)));
    FM_HIP_CHECK(hipMalloc(&g.xM8, (size_t)g.nLxAlloc * g.pEC * g.P));
    FM_HIP_CHECK(hipMalloc(&g.xMs,
                           (size_t)g.nLxAlloc * g.pEC * (g.P / 64)));
  }
  if (g.esz == 2) {
    // fused persistent kernel state: control block + per-tile arrival
    // counters (zeroed per forward by a memset node) + host-mapped
    // give-up flag
    const int nTiles = g.S / 128;
    // + per-tile logits arrivals + per-(expert, row-tile) up completion
    // counters (worst case BM=128 row tiles) + an embedded eC mirror so
    // ONE memset node re-initializes every per-forward word (a second
    // 32-B memset blit costs ~4 us of wall per step)
    g.fusedCtlBytes = sizeof(FusedCtl) + (size_t)nTiles * sizeof(uint32_t) +
                      (size_t)g.E * (g.pEC / 128) * sizeof(uint32_t) +
                      (size_t)g.E * sizeof(uint32_t);
    FM_HIP_CHECK(hipMalloc(&g.fusedCtl, g.fusedCtlBytes));
    FM_HIP_CHECK(hipMemset(g.fusedCtl, 0, g.fusedCtlBytes));
    FM_HIP_CHECK(hipHostMalloc(&g.hFusedErr, sizeof(uint32_t),
                               hipHostMallocMapped));
    *g.hFusedErr = 0;
    FM_HIP_CHECK(hipHostGetDevicePointer(
        reinterpret_cast<void**>(&g.dFusedErr), g.hFusedErr, 0));
    int dev = 0;
    FM_HIP_CHECK(hipGetDevice(&dev));
    int ncu = 0;
    FM_HIP_CHECK(hipDeviceGetAttribute(
        &ncu, hipDeviceAttributeMultiprocessorCount, dev));
    g.nCU = ncu;
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) ==
            hipSuccess && khz > 0)
      g.wallClockKHz = khz;
  }
  g.initialized = true;
  return FM_OK;
}

int fm_finalize(void) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  if (g.graphExec) { (void)hipGraphExecDestroy(g.graphExec); g.graphExec = nullptr; }
  (void)hipFree(g.tokenIds); (void)hipFree(g.eC); (void)hipFree(g.xM);
  (void)hipFree(g.O32);
  (void)hipFree(g.cbuf); (void)hipFree(g.kept);
  if (g.sliceExpert) (void)hipFree(g.sliceExpert);
  (void)hipFree(g.logits32); (void)hipFree(g.gML);
  if (g.gateCtl) (void)hipFree(g.gateCtl);
  if (g.x8) { (void)hipFree(g.x8); (void)hipFree(g.xs);
              (void)hipFree(g.xM8); (void)hipFree(g.xMs); }
  if (g.fusedCtl) (void)hipFree(g.fusedCtl);
  if (g.hFusedErr) (void)hipHostFree(g.hFusedErr);
  if (g.heap) {
    for (int p = 0; p < g.world; ++p) {
      // close only real IPC mappings: a NULL-handle connect aliases
      // peers to the local heap, and closing that poisons the sticky
      // per-thread HIP error state for later launches
      if (g.peerOpened[p]) (void)hipIpcCloseMemHandle(g.peerBase[p]);
    }
    (void)hipFree(g.heap); (void)hipFree(g.dPeerRecv); (void)hipFree(g.dArrive);
    if (g.hP2pErr) (void)hipHostFree(g.hP2pErr);
  }
  g = State{};
  return FM_OK;
}

int fm_get_compiled_config(int64_t* S, int64_t* H, int64_t* E, int64_t* P,
                           int64_t* PX, int64_t* element_size) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  if (S) *S = g.S;
  if (H) *H = g.H;
  if (E) *E = g.E;
  if (P) *P = g.P;
  if (PX) *PX = g.PX;
  if (element_size) *element_size = (int64_t)g.esz;
  return FM_OK;
}

int fm_get_num_local_experts(void) { return g.initialized ? g.nLx : -1; }

int fm_get_num_shared_experts(void) { return g.initialized ? g.nSh : -1; }

int fm_last_forward_fused(void) {
  return g.initialized ? (g.lastForwardFused ? 1 : 0) : -1;
}

int fm_last_forward_decode_ffn(void) {
  return g.initialized ? (g.lastForwardDecodeFfn ? 1 : 0) : -1;
}

int fm_set_router(const fm_router_config* r) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  const fm_router_config def = State{}.router;
  const fm_router_config c = r ? *r : def;
  const int E = g.E, k = g.cfg.expert_top_k;
#define FM_ROUTER_REFUSE(...)                                                 \
  do {                                                                        \
    snprintf(g_err, sizeof(g_err), __VA_ARGS__);                              \
    return FM_ERR_UNSUPPORTED;                                                \
  } while (0)
  if (c.scoring_func != 0 && c.scoring_func != 1)
    FM_ROUTER_REFUSE("scoring_func must be 0 (softmax) or 1 (sigmoid); got %d",
                     c.scoring_func);
  if (c.norm_topk_prob != 0 && c.norm_topk_prob != 1)
    FM_ROUTER_REFUSE("norm_topk_prob must be 0 or 1; got %d", c.norm_topk_prob);
  if (c.group_score != 0 && c.group_score != 1)
    FM_ROUTER_REFUSE("group_score must be 0 (max) or 1 (sum of top 2); got %d",
                     c.group_score);
  if (c.n_group < 1 || c.n_group > kMaxGroups)
    FM_ROUTER_REFUSE("n_group must be in [1, %d]; got %d", kMaxGroups,
                     c.n_group);
  if (E % c.n_group)
    FM_ROUTER_REFUSE("num_experts = %d is not divisible by n_group = %d", E,
                     c.n_group);
  if (c.topk_group < 1 || c.topk_group > c.n_group)
    FM_ROUTER_REFUSE("topk_group must be in [1, n_group = %d]; got %d",
                     c.n_group, c.topk_group);
  if (k > c.topk_group * (E / c.n_group))
    FM_ROUTER_REFUSE("expert_top_k = %d exceeds the topk_group * E / n_group = "
                     "%d experts of the kept groups", k,
                     c.topk_group * (E / c.n_group));
  if (c.group_score == 1 && E / c.n_group < 2)
    FM_ROUTER_REFUSE("group_score 1 (sum of top 2) needs at least 2 experts "
                     "per group; n_group = %d leaves %d", c.n_group,
                     E / c.n_group);
  if (!std::isfinite(c.routed_scaling_factor) ||
      !(c.routed_scaling_factor > 0.0f))
    FM_ROUTER_REFUSE("routed_scaling_factor must be finite and > 0; got %g",
                     (double)c.routed_scaling_factor);
  if (k == 1 && c.norm_topk_prob == 0)
    FM_ROUTER_REFUSE("norm_topk_prob 0 is not supported with expert_top_k 1: "
                     "the top-1 direct store is unscaled");
  if (k == 1 && c.routed_scaling_factor != 1.0f)
    FM_ROUTER_REFUSE("routed_scaling_factor != 1 is not supported with "
                     "expert_top_k 1: the top-1 direct store is unscaled");
  const bool rv = c.scoring_func != def.scoring_func ||
                  c.norm_topk_prob != def.norm_topk_prob ||
                  c.n_group != def.n_group || c.topk_group != def.topk_group ||
                  c.group_score != def.group_score ||
                  c.routed_scaling_factor != def.routed_scaling_factor ||
                  c.score_bias != nullptr;
  if (rv && g.cfg.is_training) {
    const char* key = c.scoring_func != 0 ? "scoring_func"
                      : c.norm_topk_prob != 1 ? "norm_topk_prob"
                      : c.n_group != 1 ? "n_group"
                      : c.topk_group != 1 ? "topk_group"
                      : c.group_score != 0 ? "group_score"
                      : c.routed_scaling_factor != 1.0f ? "routed_scaling_factor"
                                                        : "score_bias";
    FM_ROUTER_REFUSE("a non-default %s is not supported with is_training 1: "
                     "the aux-loss accumulators are softmax-specific", key);
  }
  if (E > 256 && (c.scoring_func == 1 || c.score_bias || c.n_group > 1)) {
    const char* key = c.scoring_func == 1 ? "scoring_func 1"
                      : c.score_bias ? "score_bias" : "n_group > 1";
    FM_ROUTER_REFUSE("%s is not supported with num_experts > 256 (the route "
                     "kernel's LDS budget); norm_topk_prob and "
                     "routed_scaling_factor work at every E", key);
  }
#undef FM_ROUTER_REFUSE
  g.router = c;
  g.routerRV = rv;
  ++g.routerGen;  // never replay a forward captured under another router
  return FM_OK;
}

int fm_set_weight_scales(const float* scales, int32_t granularity) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  if (granularity == 2) {
    setErr("weight scale granularity 2 (128x128 blocks) is reserved: block "
           "scales vary along K and need in-loop handling (DESIGN.md 5l)");
    return FM_ERR_UNSUPPORTED;
  }
  if (granularity != 0 && granularity != 1) {
    snprintf(g_err, sizeof(g_err),
             "weight scale granularity must be 0 (none) or 1 (per output "
             "channel); got %d", (int)granularity);
    return FM_ERR_UNSUPPORTED;
  }
  if (granularity == 1 && g.cfg.dtype != 4 && g.cfg.dtype != 5) {
    snprintf(g_err, sizeof(g_err),
             "weight scales need fp8 expert weights: torch_dtype must be 4 or "
             "5, the config has torch_dtype %d", (int)g.cfg.dtype);
    return FM_ERR_UNSUPPORTED;
  }
  if (granularity == 1 && !scales) {
    setErr("null weight scales with granularity 1");
    return FM_ERR_STATE;
  }
  g.wScale = granularity == 1 ? scales : nullptr;
  g.wScaleGran = granularity;
  ++g.wScaleGen;  // never replay a forward captured under other scales
  return FM_OK;
}

int fm_get_weight_scales(const float** scales, int32_t* granularity) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  if (scales) *scales = g.wScale;
  if (granularity) *granularity = g.wScaleGran;
  return FM_OK;
}

int fm_get_router(fm_router_config* out) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  if (!out) { setErr("null router config"); return FM_ERR_STATE; }
  *out = g.router;
  return FM_OK;
}

static int launch_group_gemm(hipStream_t st, int phase, const GemmArgs& a,
                             int M, int nE) {
  const int act = (phase == 0) ? a.act : 0;
  // gated up phase (hidden_act 2/3; never dtype 5, fm_initialize refuses
  // it): the callers describe the plain [P, H] problem; the kernels run
  // it over the effective N = 2P (tile-local B rows interleaved from Wglu
  // and Wup) and store P columns. Grid, job counts and the mode
  // thresholds below all see the effective N.
  const bool gated = act >= 2;
  const bool hasBias = a.bias != nullptr;
  if (gated && hasBias) {  // every up launch passes here
    setErr("b_up is not supported with a gated hidden_act (2/3)");
    return FM_ERR_UNSUPPORTED;
  }
  const int N = gated ? 2 * a.N : a.N;
  // slot 0 (Wup, at B) -> slot 2 (Wglu), in weight elements
  const long long gluOffset = gated ? 2LL * a.N * a.K : 0;
  if (g.cfg.dtype == 5 && phase != 3) {
    // MX fp8 grouped GEMM (the gate-logits GEMM stays bf16: gate_w is
    // Element-typed). 256x256 tile when the shape affords it (staging
    // bytes/flop halve: the 128^2 MX tile is glds-rate-bound at ~140
    // GB/s/CU demand vs the ~108 measured ceiling); 128^2 otherwise.
    // Persistent grid amortizes per-job setup.
    GemmArgs aa = a;
    aa.splitK = 1;
    aa.totalJobs = 0;
    // geometry: 128x256 triple-buffered is the measured default
    // wherever N affords 256-wide tiles (cfg3/4/5 shapes: -7..-12% -
    // the 2-stage pipeline's per-tile drain was the stall,
    // profiles/r02_mx_pmc.txt; the 256^2 SE2 tile halves B re-reads but
    // loses more to latency, kept behind FM_MX_GEOM=big for A/B);
    // 128^2 for narrow N
    static const int forceBig = [] {
      const char* e2 = getenv("FM_MX_GEOM");
      return (e2 && e2[0] == 'b') ? 1 : 0;
    }();
    const bool big = forceBig && mxBigGeom(M, N, nE);
    const bool mid = !big && (N >= 256) &&
                     DIVUP(M, 128) * DIVUP(N, 256) * nE >=
                         (g.nCU > 0 ? g.nCU : 256);
    const int bm = big ? 256 : 128, bn = (big || mid) ? 256 : 128;
    static const bool mxS3 = [] {
      const char* e2 = getenv("FM_MX_STAGES");
      return !(e2 && e2[0] == '2');
    }();
    dim3 grid(DIVUP(M, bm), DIVUP(N, bn), nE);
    dim3 block(512);
    {
      const int J = grid.x * grid.y * nE;
      const int resident = (big ? 1 : 2) * (g.nCU > 0 ? g.nCU : 256);
      if (J > resident) {
        aa.totalJobs = J;
        aa.jobsMT = grid.x;
        aa.jobsNT = grid.y;
        grid = dim3(resident, 1, 1);
      }
    }
#define MXGG(PH, AC, HB)                                                      \
    do {                                                                      \
      if (big)                                                                \
        hipLaunchKernelGGL((k_group_gemm_mx<PH, AC, HB, 256, 256>), grid,     \
                           block, 0, st, aa);                                 \
      else if (mid && mxS3)                                                   \
        hipLaunchKernelGGL((k_group_gemm_mx<PH, AC, HB, 128, 256, 3>), grid,  \
                           block, 0, st, aa);                                 \
      else if (mid)                                                           \
        hipLaunchKernelGGL((k_group_gemm_mx<PH, AC, HB, 128, 256>), grid,     \
                           block, 0, st, aa);                                 \
      else                                                                    \
        hipLaunchKernelGGL((k_group_gemm_mx<PH, AC, HB, 128, 128>), grid,     \
                           block, 0, st, aa);                                 \
    } while (0)
    const int sel = phase * 4 + act * 2 + (hasBias ? 1 : 0);
    switch (sel) {
      case 0: MXGG(0, 0, false); break;
      case 1: MXGG(0, 0, true); break;
      case 2: MXGG(0, 1, false); break;
      case 3: MXGG(0, 1, true); break;
      case 4: MXGG(1, 0, false); break;
      case 5: MXGG(1, 0, true); break;
      default:
        if (hasBias) MXGG(2, 0, true);
        else MXGG(2, 0, false);
        break;
    }
#undef MXGG
    FM_HIP_CHECK(hipGetLastError());
    return FM_OK;
  }
  if (g.esz == 2) {
    // tile selection: prefer the deep-pipelined 256-row kernel when the
    // grid still fills the 256 CUs at 1 block/CU. When BN=256 alone
    // cannot fill the chip (small N, e.g. the down GEMM at H=1024), the
    // fp32-atomic combine epilogue makes K-split partials free, so
    // split-K restores occupancy at BN=256's lower staging traffic.
    const int b256 = DIVUP(M, 256) * DIVUP(N, 256) * nE;
    const int b128n = DIVUP(M, 256) * DIVUP(N, 128) * nE;
    const int h256 = DIVUP(M, 128) * DIVUP(N, 256) * nE;  // BM=128 rows
    const int h128 = DIVUP(M, 128) * DIVUP(N, 128) * nE;
    // modes: 0 big(BMxBN 256x256), 1 big(256x128), 3 big(128x256),
    // 4 big(128x128), 2 small synchronous 128x128. Prefer the largest
    // tile whose grid still fills the chip; the BM=128 pipelined tiles
    // cover the many-experts shapes where per-expert M == pEC == 128
    // (configs 3-5 shapes and the EP segments).
    // NOTE: split-K via the atomic combine epilogue is wired up
    // (a.splitK) but DISABLED by default: at config 2 it doubled the
    // 8.3M fp32 atomics and cost more (+13 us) than the BN=256 staging
    // saving bought (profiles/r01). Revisit for huge-K shapes.
    int mode;
    int skf = 1;
    static const int forceMode = [] {
      const char* e = getenv("FM_FORCE_MODE");
      return e ? atoi(e) : -1;
    }();
    static const int noRemap = [] {
      const char* e = getenv("FM_NO_REMAP");
      return (e && e[0] == '1') ? 1 : 0;
    }();
    if (M >= 256 && b256 >= 256) mode = 0;
    // 128x128 runs 2 blocks/CU (65 KB LDS, 71 VGPR) so block-level
    // overlap hides the per-tile sync; prefer it over the BN=128 /
    // BM=128 single-resident tiles whenever the grid can fill 2/CU AND
    // K is not huge (at K=14336 the 1.33x staging of the smaller tile
    // outweighs the overlap - measured on the cfg4 shape). Checked
    // BEFORE mode 1: the cfg2 down GEMM (M=N=1024) runs 69 us in mode 4
    // vs 73 us in mode 1 (measured).
    else if (M >= 128 && h128 >= 512 && a.K <= 8192) mode = 4;
    else if (M >= 256 && b128n >= 256) mode = 1;
    else if (M >= 128 && h256 >= 256) mode = 3;
    else if (M >= 128 && h128 >= 256) mode = 4;
    else mode = 2;
    if (forceMode >= 0) mode = forceMode;
    GemmArgs aa = a;
    aa.N = N;
    aa.gluOffset = gluOffset;
    aa.splitK = skf;
    aa.noRemap = noRemap;
    aa.totalJobs = 0;
    const int bmSel = (mode == 0 || mode == 1) ? 256 : 128;
    const int bnSel = (mode == 0 || mode == 3) ? 256 : 128;
    dim3 block(mode == 2 ? 256 : 512);
    dim3 grid(DIVUP(M, mode == 2 ? 128 : bmSel),
              DIVUP(N, mode == 2 ? 128 : bnSel), nE * skf);
    // persistent grid for the big-tile modes: launch exactly the number
    // of co-resident blocks (1/CU for the 1-block modes, 2/CU for the
    // 128^2 tile) and let each walk several (m,n,e) tiles - amortizes
    // the per-block setup + prologue staging bubble (measured ~19 us of
    // the 71 us cfg2 up kernel). FM_PERSIST=0 reverts to 1 tile/block.
    static const bool persist = [] {
      const char* e = getenv("FM_PERSIST");
      return !(e && e[0] == '0');
    }();
    // FM_PERSIST_BLOCKS=<n> caps the persistent grid at n blocks (test
    // knob: one block then walks many jobs at a small shape)
    static const int persistCap = [] {
      const char* e = getenv("FM_PERSIST_BLOCKS");
      return e ? atoi(e) : 0;
    }();
    if (persist && mode != 2) {
      const int jm = grid.x, jn = grid.y, J = jm * jn * nE * skf;
      int resident = (mode == 4) ? 512 : 256;
      if (persistCap > 0) resident = std::min(resident, persistCap);
      if (J > resident) {
        aa.totalJobs = J;
        aa.jobsMT = jm;
        aa.jobsNT = jn;
        grid = dim3(resident, 1, 1);
      }
    }
    if (phase == 3) {  // gate logits (fp32 out, B = gate_w)
      // big-E shapes (e.g. cfg5: S=16384, E=256) fill the chip with the
      // pipelined 128x128 tile (zeroing of eC still needs the small
      // kernel's block-0 path, so hand that to a tiny memset instead)
      // (a decode-sized forward, M < 128, always takes the small kernel:
      // its TAILA instantiation clamps the ragged x rows)
      if (mode != 2 && N >= 128 && M >= 128) {
        GemmArgs a3 = a;
        a3.splitK = 1;
        a3.noRemap = noRemap;
        a3.totalJobs = 0;
        if (a3.eC)  // PHASE 3 big kernel does not zero eC; do it here
          FM_HIP_CHECK(hipMemsetAsync(const_cast<uint32_t*>(a3.eC), 0,
                                      (size_t)a3.EC * sizeof(uint32_t), st));
        // K-split to fill the chip when the logits tile grid is narrow
        // (cfg5: 128 x 2 tiles left half the CUs idle): partials
        // atomicAdd into logits32, which is kept zero between forwards
        // by the route's re-zeroing pass
        {
          const int b3 = DIVUP(M, bmSel) * DIVUP(N, bnSel);
          while (a3.splitK < 8 && b3 * a3.splitK * 2 <= 512 &&
                 (a.K / 64) % (a3.splitK * 2) == 0)
            a3.splitK *= 2;
          a3.atomicLogits = (a3.splitK > 1) ? 1 : 0;
        }
        dim3 g3(DIVUP(M, bmSel), DIVUP(N, bnSel), a3.splitK);
        if (g.cfg.dtype == 3) {
          if (mode == 0)
            hipLaunchKernelGGL((k_group_gemm_bf16_big<fp16, 3, 0, false, 256, 256>), g3, dim3(512), 0, st, a3);
          else if (mode == 1)
            hipLaunchKernelGGL((k_group_gemm_bf16_big<fp16, 3, 0, false, 128, 256>), g3, dim3(512), 0, st, a3);
          else if (mode == 3)
            hipLaunchKernelGGL((k_group_gemm_bf16_big<fp16, 3, 0, false, 256, 128>), g3, dim3(512), 0, st, a3);
          else
            hipLaunchKernelGGL((k_group_gemm_bf16_big<fp16, 3, 0, false, 128, 128>), g3, dim3(512), 0, st, a3);
        } else {
          if (mode == 0)
            hipLaunchKernelGGL((k_group_gemm_bf16_big<bf16, 3, 0, false, 256, 256>), g3, dim3(512), 0, st, a3);
          else if (mode == 1)
            hipLaunchKernelGGL((k_group_gemm_bf16_big<bf16, 3, 0, false, 128, 256>), g3, dim3(512), 0, st, a3);
          else if (mode == 3)
            hipLaunchKernelGGL((k_group_gemm_bf16_big<bf16, 3, 0, false, 256, 128>), g3, dim3(512), 0, st, a3);
          else
            hipLaunchKernelGGL((k_group_gemm_bf16_big<bf16, 3, 0, false, 128, 128>), g3, dim3(512), 0, st, a3);
        }
        FM_HIP_CHECK(hipGetLastError());
        return FM_OK;
      }
      // small-E: 128^2 kernel with K-split to fill the chip (the logits
      // grid is only S/128 x E/128 blocks)
      const int b3 = DIVUP(M, 128) * DIVUP(N, 128);
      int sk3 = 1;
      while (sk3 < 8 && b3 * sk3 * 2 <= 512 && (a.K / 64) % (sk3 * 2) == 0)
        sk3 *= 2;
      GemmArgs a3 = a;
      a3.splitK = sk3;
      // logits32 is zero on entry (zeroed at initialize and re-zeroed by
      // k_gate_route after each read)
      dim3 g3(DIVUP(M, 128), DIVUP(N, 128), sk3);
      if (M < 128 && g.cfg.dtype == 3)
        hipLaunchKernelGGL((k_group_gemm_bf16<fp16, 3, 0, false, fp16, true>),
                           g3, dim3(256), 0, st, a3);
      else if (M < 128)
        hipLaunchKernelGGL((k_group_gemm_bf16<bf16, 3, 0, false, bf16, true>),
                           g3, dim3(256), 0, st, a3);
      else if (g.cfg.dtype == 3)
        hipLaunchKernelGGL((k_group_gemm_bf16<fp16, 3, 0, false>), g3,
                           dim3(256), 0, st, a3);
      else
        hipLaunchKernelGGL((k_group_gemm_bf16<bf16, 3, 0, false>), g3,
                           dim3(256), 0, st, a3);
      FM_HIP_CHECK(hipGetLastError());
      return FM_OK;
    }
    const int sel = phase * 4 + act * 2 + (hasBias ? 1 : 0);
    // modes 1/3 (the 128-wide tiles) run the triple-buffered staging
    // pipeline by default (LDS 144 KB; counted vmcnt waits, two compute
    // phases of staging latency budget); FM_STAGES=2 reverts for A/B
    // comparison. Modes 0/4 keep double buffering (LDS / occupancy).
    static const bool s3 = [] {
      const char* e = getenv("FM_STAGES");
      return !(e && e[0] == '2');
    }();
#define GG_ET(ET, PH, AC, HB, WET)                                            \
    do {                                                                      \
      if (mode == 0)  /* triple measured -5% here even for fp8 B */          \
        hipLaunchKernelGGL(                                                   \
            (k_group_gemm_bf16_big<ET, PH, AC, HB, 256, 256, WET>),           \
            grid, block, 0, st, aa);                                          \
      else if (mode == 1 && s3)                                               \
        hipLaunchKernelGGL(                                                   \
            (k_group_gemm_bf16_big<ET, PH, AC, HB, 128, 256, WET, 3>),        \
            grid, block, 0, st, aa);                                          \
      else if (mode == 1)                                                     \
        hipLaunchKernelGGL(                                                   \
            (k_group_gemm_bf16_big<ET, PH, AC, HB, 128, 256, WET>),           \
            grid, block, 0, st, aa);                                          \
      else if (mode == 3 && s3)                                               \
        hipLaunchKernelGGL(                                                   \
            (k_group_gemm_bf16_big<ET, PH, AC, HB, 256, 128, WET, 3>),        \
            grid, block, 0, st, aa);                                          \
      else if (mode == 3)                                                     \
        hipLaunchKernelGGL(                                                   \
            (k_group_gemm_bf16_big<ET, PH, AC, HB, 256, 128, WET>),           \
            grid, block, 0, st, aa);                                          \
      else if (mode == 4)                                                     \
        hipLaunchKernelGGL(                                                   \
            (k_group_gemm_bf16_big<ET, PH, AC, HB, 128, 128, WET>),           \
            grid, block, 0, st, aa);                                          \
      else                                                                    \
        hipLaunchKernelGGL((k_group_gemm_bf16<ET, PH, AC, HB, WET>), grid,    \
                           block, 0, st, aa);                                 \
    } while (0)
#define GG_CASE(PH, AC, HB)                                                   \
    do {                                                                      \
      if (g.cfg.dtype == 3) GG_ET(fp16, PH, AC, HB, fp16);                    \
      else if (g.cfg.dtype == 4) GG_ET(bf16, PH, AC, HB, fp8e4m3);            \
      else GG_ET(bf16, PH, AC, HB, bf16);                                     \
    } while (0)
    // gated (phase 0, bias-free by contract): ACT 2 SwiGLU / 3 GeGLU
    if (gated) {
      if (act == 2) GG_CASE(0, 2, false);
      else GG_CASE(0, 3, false);
    } else switch (sel) {
      case 0: GG_CASE(0, 0, false); break;
      case 1: GG_CASE(0, 0, true); break;
      case 2: GG_CASE(0, 1, false); break;
      case 3: GG_CASE(0, 1, true); break;
      case 4: GG_CASE(1, 0, false); break;
      case 5: GG_CASE(1, 0, true); break;
      default:
        if (hasBias) GG_CASE(2, 0, true);
        else GG_CASE(2, 0, false);
        break;
    }
#undef GG_CASE
  } else {
    dim3 block(256);
    dim3 grid(DIVUP(M, 64), DIVUP(N, 64), nE);
    if (gated) {
      GemmArgs aa = a;
      aa.N = N;
      aa.gluOffset = gluOffset;
      if (act == 2)
        hipLaunchKernelGGL((k_group_gemm_f32<0, 2, false>), grid, block, 0, st, aa);
      else
        hipLaunchKernelGGL((k_group_gemm_f32<0, 3, false>), grid, block, 0, st, aa);
      FM_HIP_CHECK(hipGetLastError());
      return FM_OK;
    }
    const int sel = phase * 4 + act * 2 + (hasBias ? 1 : 0);
    switch (sel) {
      case 0: hipLaunchKernelGGL((k_group_gemm_f32<0, 0, false>), grid, block, 0, st, a); break;
      case 1: hipLaunchKernelGGL((k_group_gemm_f32<0, 0, true>), grid, block, 0, st, a); break;
      case 2: hipLaunchKernelGGL((k_group_gemm_f32<0, 1, false>), grid, block, 0, st, a); break;
      case 3: hipLaunchKernelGGL((k_group_gemm_f32<0, 1, true>), grid, block, 0, st, a); break;
      case 4: hipLaunchKernelGGL((k_group_gemm_f32<1, 0, false>), grid, block, 0, st, a); break;
      case 5: hipLaunchKernelGGL((k_group_gemm_f32<1, 0, true>), grid, block, 0, st, a); break;
      default:
        if (hasBias) hipLaunchKernelGGL((k_group_gemm_f32<2, 0, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_group_gemm_f32<2, 0, false>), grid, block, 0, st, a);
        break;
    }
  }
  FM_HIP_CHECK(hipGetLastError());
  return FM_OK;
}

// FM_DECODE_FFN: 0 forces the grouped GEMMs at a decode size, 1 forces the
// weight-streaming kernels, unset takes the measured default. Re-read per
// call (tests toggle it) and part of the graph key, like FM_FUSED.
static int decodeFfnMode() {
  const char* e = getenv("FM_DECODE_FFN");
  return (e && (e[0] == '0' || e[0] == '1')) ? e[0] - '0' : -1;
}

// does a forward take k_decode_ffn? Only below 128 tokens, and only for the
// 2-byte activation families (fp32 stays on k_group_gemm_f32).
static bool decodeFfnApplies() {
  if (g.S >= 128 || g.esz != 2 || g.cfg.dtype == 5) return false;
  const int m = decodeFfnMode();
  if (m >= 0) return m == 1;
  return g.S <= (g.cfg.dtype == 4   ? kDecodeFfnMaxSFp8
                 : g.cfg.dtype == 3 ? kDecodeFfnMaxSFp16
                                    : kDecodeFfnMaxSBf16);
}

// one launch of k_decode_ffn over all z-slices: 16 weight rows per block
static int launch_decode_ffn(hipStream_t st, int phase, const GemmArgs& a,
                             int nZ) {
  const bool gated = phase == 0 && a.act >= 2;
  if (gated && a.bias) {
    setErr("b_up is not supported with a gated hidden_act (2/3)");
    return FM_ERR_UNSUPPORTED;
  }
  GemmArgs aa = a;
  aa.gluOffset = gated ? 2LL * a.N * a.K : 0;  // Wup (slot 0) -> Wglu (slot 2)
  const dim3 grid(a.N / 16, nZ), block(256);
#define DEC_ET(ET, WET, WS)                                                   \
  do {                                                                        \
    if (phase == 1)                                                           \
      hipLaunchKernelGGL((k_decode_ffn<ET, WET, 1, false, WS>), grid, block,  \
                         0, st, aa);                                          \
    else if (gated)                                                           \
      hipLaunchKernelGGL((k_decode_ffn<ET, WET, 0, true, WS>), grid, block,   \
                         0, st, aa);                                          \
    else                                                                      \
      hipLaunchKernelGGL((k_decode_ffn<ET, WET, 0, false, WS>), grid, block,  \
                         0, st, aa);                                          \
  } while (0)
  if (g.cfg.dtype == 3) DEC_ET(fp16, fp16, false);
  else if (g.cfg.dtype == 4 && aa.wScale) DEC_ET(bf16, fp8e4m3, true);
  else if (g.cfg.dtype == 4) DEC_ET(bf16, fp8e4m3, false);
  else DEC_ET(bf16, bf16, false);
#undef DEC_ET
  FM_HIP_CHECK(hipGetLastError());
  return FM_OK;
}

static int launch_cast_combine(hipStream_t st, void* moe_out) {
  // tokens per block iteration (mirrors the kernel): H / (16 / esz) chunks
  const int cpt = std::max(1, g.H / (16 / (int)g.esz));
  const int tpb = cpt < 256 ? 256 / cpt : 1;
  const int blocks = std::min(DIVUP(g.S, tpb), 4096);
#define CC(T, KK)                                                             \
  hipLaunchKernelGGL((k_cast_combine<T, KK>), dim3(blocks), dim3(256), 0, st, \
                     reinterpret_cast<const T*>(g.cbuf), g.kept,              \
                     reinterpret_cast<T*>(moe_out), g.S, g.H)
#define CCS(T, KK)                                                            \
  hipLaunchKernelGGL((k_cast_combine_shared<T, KK>), dim3(blocks), dim3(256), \
                     0, st, reinterpret_cast<const T*>(g.cbuf), g.kept,       \
                     reinterpret_cast<T*>(moe_out), g.S, g.H, g.nSh)
  // shared experts: the [S, k + nSh, H] sibling (k == 1 included)
#define CCS_K(T)                                                              \
  switch (g.cfg.expert_top_k) {                                               \
    case 1: CCS(T, 1); break;                                                 \
    case 2: CCS(T, 2); break;                                                 \
    case 3: CCS(T, 3); break;                                                 \
    case 4: CCS(T, 4); break;                                                 \
    case 5: CCS(T, 5); break;                                                 \
    case 6: CCS(T, 6); break;                                                 \
    case 7: CCS(T, 7); break;                                                 \
    case 8: CCS(T, 8); break;                                                 \
    default: setErr("bad topk"); return FM_ERR_UNSUPPORTED;                   \
  }
  if (g.nSh > 0) {
    if (g.cfg.dtype == 3) { CCS_K(fp16) }
    else if (g.esz == 2) { CCS_K(bf16) }
    else { CCS_K(float) }
    FM_HIP_CHECK(hipGetLastError());
    return FM_OK;
  }
#define CC_K(T)                                                               \
  switch (g.cfg.expert_top_k) {                                               \
    case 2: CC(T, 2); break;                                                  \
    case 3: CC(T, 3); break;                                                  \
    case 4: CC(T, 4); break;                                                  \
    case 5: CC(T, 5); break;                                                  \
    case 6: CC(T, 6); break;                                                  \
    case 7: CC(T, 7); break;                                                  \
    case 8: CC(T, 8); break;                                                  \
    default: setErr("bad topk"); return FM_ERR_UNSUPPORTED;                   \
  }
  if (g.cfg.dtype == 3) { CC_K(fp16) }
  else if (g.esz == 2) { CC_K(bf16) }
  else { CC_K(float) }
#undef CC_K
#undef CCS_K
#undef CCS
#undef CC
  FM_HIP_CHECK(hipGetLastError());
  return FM_OK;
}

// dtype 5: quantize bf16 rows into fp8 + per-64 block scales
static int launch_quant_mx(hipStream_t st, const void* in, uint8_t* out,
                           uint8_t* scales, long long nRows, int K) {
  const long long nBlk = nRows * (K / 64);
  const int grid = (int)std::min<long long>(DIVUP(nBlk, 4), 8192);
  hipLaunchKernelGGL(k_quant_mx<bf16>, dim3(grid), dim3(256), 0, st,
                     reinterpret_cast<const bf16*>(in), out, scales, nRows,
                     K);
  FM_HIP_CHECK(hipGetLastError());
  return FM_OK;
}

static int moe_forward_impl(hipStream_t st, const void* x, const void* gate_w,
                            const void* expert_w, const void* b_up,
                            const void* b_dn, void* gate_out, void* moe_out,
                            int64_t S, hipEvent_t* evs) {
  // fused single-launch path (the north-star structure); classic
  // multi-kernel path remains for fp32 and as FM_FUSED=0 fallback
  g.lastForwardFused = false;
  g.lastForwardDecodeFfn = false;
  if (b_up && g.gated) {  // refuse before anything is enqueued
    setErr("b_up is not supported with a gated hidden_act (2/3)");
    return FM_ERR_UNSUPPORTED;
  }
  // gated experts never take the fused kernel: its down-walk arrival
  // counts are keyed on the number of up N-tiles
  // (nor do configs with shared experts: the fused walks know E experts)
  // (nor does a non-default router: k_moe_fused routes with the legacy
  // route_tile_core)
  // (nor does a decode-sized forward, S < 128: no ragged tile there)
  // (nor does a forward with weight scales attached: k_moe_fused is not
  // taught about them, its GemmArgs carry none)
  if (fusedEnabled() && g.S >= 128 && g.esz == 2 && g.world == 1 &&
      g.cfg.dtype != 5 && !g.gated && g.nSh == 0 && !g.routerRV &&
      !g.wScale) {
    int rc = moe_forward_fused(st, x, gate_w, expert_w, b_up, b_dn, gate_out,
                               moe_out);
    if (rc != FM_FALLBACK) {
      if (rc == FM_OK) g.lastForwardFused = true;
      return rc;
    }
  }
  // eC is written by the gate itself (k_gate_fused publishes it whole;
  // the two-kernel gate zeroes it in the logits kernel's block 0)
  // O32 is kept zero across calls (zeroed at initialize; k_cast_out
  // re-zeroes after reading)
  // k==1: zero moe_out so dropped tokens keep zeros (clearState,
  // moe.cuh:30-70); k>1 writes every element via k_cast_out instead
  // (shared experts: k==1 goes through the combine slots too, and the
  // combine writes every element - no memset)
  if (g.cfg.expert_top_k == 1 && g.nSh == 0) {
    FM_HIP_CHECK(hipMemsetAsync(moe_out, 0, (size_t)g.S * g.H * g.esz, st));
  }
  if (evs) FM_HIP_CHECK(hipEventRecord(evs[1], st));

  int rc = launch_gate(st, x, gate_w, gate_out, S);
  if (rc != FM_OK) return rc;
  if (evs) FM_HIP_CHECK(hipEventRecord(evs[2], st));

  if (g.cfg.dtype == 5) {
    // MX: quantize the activations once; the gate above read bf16 x
    rc = launch_quant_mx(st, x, g.x8, g.xs, g.S, g.H);
    if (rc != FM_OK) return rc;
  }

  GemmArgs up{};
  up.A = (g.cfg.dtype == 5) ? (const void*)g.x8 : x;
  up.aScales = g.xs;
  up.B = expert_w;
  up.bias = b_up;
  up.out = g.xM;
  up.gate_out = gate_out;
  up.tokenIds = g.tokenIds;
  up.eC = g.eC;
  up.strideAExpert = 0;
  up.strideBExpert = (long long)g.wMats * g.P * g.H;
  up.strideOExpert = (long long)g.pEC * g.P;
  up.K = g.H; up.N = g.P;
  up.EC = g.EC; up.pEC = g.pEC; up.PX = g.PX;
  up.topk = g.cfg.expert_top_k; up.act = g.cfg.hidden_act;
  up.expertOffset = 0; up.nRows = 0; up.H = g.H;
  setWeightScaleArgs(up, 0, 0, true);
  // shared experts ride both launches as nV extra z-slices (static routing
  // tail, fm_initialize); null map / zero counts when there are none
  const int nZ = g.E + g.nV;
  if (g.nSh > 0) {
    up.segExpert = g.sliceExpert;
    up.nShared = g.nSh;
    up.nRoutedE = g.E;
    up.slotAlways = 1;
  }
  const bool mxEpiQuant =
      (g.cfg.dtype == 5) && mxWideN(g.pEC, g.P, g.E);
  if (mxEpiQuant) {
    up.out8 = g.xM8;       // 256-tile up epilogue quantizes in-register
    up.outScales = g.xMs;  // (skips the separate k_quant_mx xM pass)
  }
  // decode-sized forward: the weight-streaming kernels (par.5k)
  const bool decode = decodeFfnApplies();
  g.lastForwardDecodeFfn = decode;
  rc = decode ? launch_decode_ffn(st, 0, up, nZ)
              : launch_group_gemm(st, 0, up, g.pEC, nZ);
  if (rc != FM_OK) return rc;
  if (evs) FM_HIP_CHECK(hipEventRecord(evs[3], st));

  if (g.cfg.dtype == 5 && !mxEpiQuant) {
    // quantize the intermediate activations for the MX down GEMM
    rc = launch_quant_mx(st, g.xM, g.xM8, g.xMs,
                         (long long)g.E * g.pEC, g.P);
    if (rc != FM_OK) return rc;
  }

  GemmArgs dn = up;
  dn.out8 = nullptr;
  dn.outScales = nullptr;
  dn.A = (g.cfg.dtype == 5) ? (const void*)g.xM8 : g.xM;
  dn.aScales = g.xMs;
  dn.B = reinterpret_cast<const char*>(expert_w) + (size_t)g.P * g.H * g.wesz;
  dn.bias = b_dn;
  dn.out = nullptr;
  dn.O32 = reinterpret_cast<float*>(g.cbuf);  // non-atomic combine slots
  dn.moe_out = moe_out;
  dn.strideAExpert = (long long)g.pEC * g.P;
  dn.K = g.P; dn.N = g.H;
  setWeightScaleArgs(dn, 1, 0, true);
  rc = decode ? launch_decode_ffn(st, 1, dn, nZ)
              : launch_group_gemm(st, 1, dn, g.pEC, nZ);
  if (rc != FM_OK) return rc;
  if (evs) FM_HIP_CHECK(hipEventRecord(evs[4], st));

  if (g.cfg.expert_top_k > 1 || g.nSh > 0) {
    int rc2 = launch_cast_combine(st, moe_out);
    if (rc2 != FM_OK) return rc2;
  }
  return FM_OK;
}

int fm_moe_forward(void* stream, const void* x, const void* gate_w,
                   const void* expert_w, const void* b_up, const void* b_dn,
                   void* gate_out, void* moe_out, int64_t S) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  if (g.world != 1) {
    setErr("fm_moe_forward is the single-rank path; use the staged EP entry points");
    return FM_ERR_STATE;
  }
  if (S != g.S) { setErr("S mismatch vs frozen config"); return FM_ERR_SHAPE; }
  int prc = fusedPoisonCheck();  // a prior fused forward that gave up
  if (prc != FM_OK) return prc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);

  // hipGraph fast path: torch's caching allocator hands back the same
  // buffers on steady-state iterations, so after two identical calls we
  // capture the 6-launch sequence once and replay it (saves the
  // per-launch host+boundary overhead; falls back to eager whenever any
  // pointer changes or capture is unavailable).
  void* key[10] = {const_cast<void*>(x), const_cast<void*>(gate_w),
                  const_cast<void*>(expert_w), const_cast<void*>(b_up),
                  const_cast<void*>(b_dn), gate_out, moe_out,
                  reinterpret_cast<void*>(static_cast<uintptr_t>(
                      (uint64_t)g.routerGen << 40 |
                      (uint64_t)(decodeFfnMode() + 1) << 38 |
                      (uint64_t)S << 2 | (gateFusedEnabled() ? 2 : 0) |
                      (fusedEnabled() ? 1 : 0))),
                  const_cast<float*>(g.wScale),
                  reinterpret_cast<void*>(static_cast<uintptr_t>(g.wScaleGen))};
  if (g.graphValid && memcmp(key, g.graphKey, sizeof(key)) == 0) {
    if (hipGraphLaunch(g.graphExec, st) == hipSuccess) return FM_OK;
    g.graphValid = false;  // replay failed: rebuild next time
  }
  if (st != nullptr && memcmp(key, g.lastKey, sizeof(key)) == 0) {
    // second consecutive identical call: try to capture
    if (g.graphExec) { (void)hipGraphExecDestroy(g.graphExec); g.graphExec = nullptr; }
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) ==
        hipSuccess) {
      int rc = moe_forward_impl(st, x, gate_w, expert_w, b_up, b_dn, gate_out,
                                moe_out, S, nullptr);
      hipGraph_t graph = nullptr;
      hipError_t ec = hipStreamEndCapture(st, &graph);
      if (rc == FM_OK && ec == hipSuccess && graph) {
        if (hipGraphInstantiate(&g.graphExec, graph, nullptr, nullptr, 0) ==
            hipSuccess) {
          memcpy(g.graphKey, key, sizeof(key));
          g.graphValid = true;
          (void)hipGraphDestroy(graph);
          // the capture did not execute; launch the graph now
          if (hipGraphLaunch(g.graphExec, st) == hipSuccess) return FM_OK;
          g.graphValid = false;
        } else {
          (void)hipGraphDestroy(graph);
        }
      } else if (graph) {
        (void)hipGraphDestroy(graph);
      }
      if (rc != FM_OK) return rc;
      // capture succeeded as a recording but instantiate/launch failed:
      // nothing ran yet - fall through to an eager execution
    }
  }
  memcpy(g.lastKey, key, sizeof(key));
  return moe_forward_impl(st, x, gate_w, expert_w, b_up, b_dn, gate_out,
                          moe_out, S, nullptr);
}

int fm_moe_forward_phased(void* stream, const void* x, const void* gate_w,
                          const void* expert_w, const void* b_up,
                          const void* b_dn, void* gate_out, void* moe_out,
                          int64_t S, float ms[4]) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  if (g.world != 1) { setErr("single-rank path only"); return FM_ERR_STATE; }
  if (S != g.S) { setErr("S mismatch vs frozen config"); return FM_ERR_SHAPE; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipEvent_t evs[6];
  for (auto& e : evs) FM_HIP_CHECK(hipEventCreate(&e));
  FM_HIP_CHECK(hipEventRecord(evs[0], st));
  int rc = moe_forward_impl(st, x, gate_w, expert_w, b_up, b_dn, gate_out,
                            moe_out, S, evs);
  if (rc == FM_OK) {
    FM_HIP_CHECK(hipEventRecord(evs[5], st));
    FM_HIP_CHECK(hipStreamSynchronize(st));
    if (g.lastForwardFused) {
      // fused forward: phase times come from the in-kernel wall clocks
      // (one launch has no event boundaries); ms = {gate+route, up GEMM,
      // down GEMM, combine} like the classic path
      int prc = fusedPoisonCheck();
      if (prc != FM_OK) { rc = prc; }
      else {
        FusedCtl hc;
        FM_HIP_CHECK(hipMemcpy(&hc, g.fusedCtl, sizeof(hc),
                               hipMemcpyDeviceToHost));
        const double khz = (double)g.wallClockKHz;
        ms[0] = (float)((double)(hc.clk[1] - hc.clk[0]) / khz);
        ms[1] = (float)((double)(hc.clk[2] - hc.clk[1]) / khz);
        ms[2] = (float)((double)(hc.clk[3] - hc.clk[2]) / khz);
        ms[3] = (float)((double)(hc.clk[4] - hc.clk[3]) / khz);
      }
    } else {
      float pre = 0, gate = 0, upT = 0, dnT = 0, post = 0;
      (void)hipEventElapsedTime(&pre, evs[0], evs[1]);
      (void)hipEventElapsedTime(&gate, evs[1], evs[2]);
      (void)hipEventElapsedTime(&upT, evs[2], evs[3]);
      (void)hipEventElapsedTime(&dnT, evs[3], evs[4]);
      (void)hipEventElapsedTime(&post, evs[4], evs[5]);
      ms[0] = gate; ms[1] = upT; ms[2] = dnT; ms[3] = pre + post;
    }
  }
  for (auto& e : evs) (void)hipEventDestroy(e);
  return rc;
}

int fm_gate_forward(void* stream, const void* x, const void* gate_w,
                    void* gate_out, int64_t S) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  if (S != g.S) { setErr("S mismatch vs frozen config"); return FM_ERR_SHAPE; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return launch_gate(st, x, gate_w, gate_out, S);  // gate zeroes eC itself
}

int fm_read_routing(void* stream, uint32_t* routed_counts, uint32_t* token_idx,
                    float* prob_sum) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint32_t* hEC = (uint32_t*)malloc((size_t)g.E * sizeof(uint32_t));
  TPS* hT = (TPS*)malloc((size_t)g.E * g.pEC * sizeof(TPS));
  if (!hEC || !hT) { free(hEC); free(hT); setErr("oom"); return FM_ERR_HIP; }
  const uint32_t* eCsrc =
      (g.lastForwardFused && g.fusedCtl) ? fusedECPtr() : g.eC;
  hipError_t e1 = hipMemcpyAsync(hEC, eCsrc, (size_t)g.E * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost, st);
  hipError_t e2 = hipMemcpyAsync(hT, g.tokenIds,
                                 (size_t)g.E * g.pEC * sizeof(TPS),
                                 hipMemcpyDeviceToHost, st);
  hipError_t e3 = hipStreamSynchronize(st);
  if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
    free(hEC); free(hT); setErr("routing D2H failed"); return FM_ERR_HIP;
  }
  for (int e = 0; e < g.E; ++e) {
    const uint32_t r = hEC[e] < (uint32_t)g.EC ? hEC[e] : (uint32_t)g.EC;
    routed_counts[e] = r;
    for (uint32_t i = 0; i < r; ++i) {
      token_idx[(size_t)e * g.EC + i] = tpsTok(hT[(size_t)e * g.pEC + i].tokenIdx);
      prob_sum[(size_t)e * g.EC + i] = hT[(size_t)e * g.pEC + i].probSum;
    }
  }
  free(hEC); free(hT);
  return FM_OK;
}

int fm_expert_ffn(void* stream, const void* rows, const void* expert_w,
                  const void* b_up, const void* b_dn, void* out_rows,
                  int64_t n_rows, int32_t local_e) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  if (g.cfg.dtype == 5) {
    setErr("dtype 5 (MX fp8) supports fm_moe_forward only this round");
    return FM_ERR_UNSUPPORTED;
  }
  if (n_rows <= 0) return FM_OK;
  if (n_rows > (int64_t)g.nLxAlloc * g.pEC) {
    setErr("n_rows exceeds workspace"); return FM_ERR_SHAPE;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  GemmArgs up{};
  up.A = rows;
  up.B = reinterpret_cast<const char*>(expert_w) +
         (size_t)local_e * g.wMats * g.P * g.H * g.wesz;
  up.bias = b_up;
  up.out = g.xM;  // scratch [n_rows, P]
  up.tokenIds = nullptr; up.eC = nullptr;
  up.strideAExpert = 0; up.strideBExpert = 0; up.strideOExpert = 0;
  up.K = g.H; up.N = g.P; up.EC = 0; up.pEC = 0; up.PX = g.PX;
  up.topk = 1; up.act = g.cfg.hidden_act; up.expertOffset = 0;
  up.nRows = (int)n_rows; up.H = g.H;
  setWeightScaleArgs(up, 0, local_e, false);  // like B: pre-offset, stride 0
  int rc = launch_group_gemm(st, 0, up, (int)n_rows, 1);
  if (rc != FM_OK) return rc;
  // note: PHASE 0 with tokenIds==nullptr writes out[e=0 stride 0] = xM rows
  GemmArgs dn = up;
  dn.A = g.xM;
  dn.B = reinterpret_cast<const char*>(expert_w) +
         ((size_t)local_e * g.wMats + 1) * g.P * g.H * g.wesz;
  dn.bias = b_dn;
  dn.out = out_rows;
  dn.K = g.P; dn.N = g.H;
  setWeightScaleArgs(dn, 1, local_e, false);
  return launch_group_gemm(st, 2, dn, (int)n_rows, 1);
}

static size_t alignUp(size_t v, size_t a) { return (v + a - 1) / a * a; }

int fm_heap_init(void) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  if (g.heap) return FM_OK;
  const size_t cells = (size_t)g.E * g.EC * g.H * g.esz;
  g.heapRecvOff = 0;
  g.heapRetOff = alignUp(cells, 256);
  g.heapDFlagOff = alignUp(g.heapRetOff + cells, 256);
  g.heapRFlagOff = alignUp(g.heapDFlagOff + (size_t)g.E * 8, 256);
  g.heapBytes = alignUp(g.heapRFlagOff + (size_t)g.E * 8, 256);
  FM_HIP_CHECK(hipMalloc(&g.heap, g.heapBytes));
  FM_HIP_CHECK(hipMemset(g.heap, 0, g.heapBytes));
  FM_HIP_CHECK(hipMalloc(&g.dPeerRecv, 4 * (size_t)g.world * 8));
  g.dPeerRet = g.dPeerRecv + g.world;
  g.dPeerDFlag = g.dPeerRet + g.world;
  g.dPeerRFlag = g.dPeerDFlag + g.world;
  FM_HIP_CHECK(hipMalloc(&g.dArrive, 2 * (size_t)g.E * 4));
  // zero-copy timeout flag: k_await_flags sets it on a bounded-spin
  // give-up; the host reads it without a stream sync
  FM_HIP_CHECK(hipHostMalloc(&g.hP2pErr, sizeof(uint32_t),
                             hipHostMallocMapped));
  *g.hP2pErr = 0;
  FM_HIP_CHECK(hipHostGetDevicePointer(
      reinterpret_cast<void**>(&g.dP2pErr), g.hP2pErr, 0));
  return FM_OK;
}

int fm_heap_handle(void* out64) {
  if (!g.heap) { setErr("fm_heap_init first"); return FM_ERR_STATE; }
  hipIpcMemHandle_t h;
  FM_HIP_CHECK(hipIpcGetMemHandle(&h, g.heap));
  memcpy(out64, &h, sizeof(h));
  return FM_OK;
}

int fm_heap_connect(const void* handles /* world x 64B, null = local only */) {
  if (!g.heap) { setErr("fm_heap_init first"); return FM_ERR_STATE; }
  uint64_t hRecv[64], hRet[64], hDF[64], hRF[64];
  for (int p = 0; p < g.world; ++p) {
    void* base = nullptr;
    if (p == g.rank || !handles) {
      base = g.heap;
    } else {
      hipIpcMemHandle_t h;
      memcpy(&h, reinterpret_cast<const char*>(handles) + (size_t)p * 64,
             sizeof(h));
      FM_HIP_CHECK(hipIpcOpenMemHandle(&base, h,
                                       hipIpcMemLazyEnablePeerAccess));
      g.peerOpened[p] = true;
    }
    g.peerBase[p] = base;
    hRecv[p] = (uint64_t)(uintptr_t)base + g.heapRecvOff;
    hRet[p] = (uint64_t)(uintptr_t)base + g.heapRetOff;
    hDF[p] = (uint64_t)(uintptr_t)base + g.heapDFlagOff;
    hRF[p] = (uint64_t)(uintptr_t)base + g.heapRFlagOff;
  }
  FM_HIP_CHECK(hipMemcpy(g.dPeerRecv, hRecv, (size_t)g.world * 8,
                         hipMemcpyHostToDevice));
  FM_HIP_CHECK(hipMemcpy(g.dPeerRet, hRet, (size_t)g.world * 8,
                         hipMemcpyHostToDevice));
  FM_HIP_CHECK(hipMemcpy(g.dPeerDFlag, hDF, (size_t)g.world * 8,
                         hipMemcpyHostToDevice));
  FM_HIP_CHECK(hipMemcpy(g.dPeerRFlag, hRF, (size_t)g.world * 8,
                         hipMemcpyHostToDevice));
  return FM_OK;
}

int fm_heap_ptrs(void** recv, void** ret) {
  if (!g.heap) { setErr("fm_heap_init first"); return FM_ERR_STATE; }
  if (recv) *recv = g.heap + g.heapRecvOff;
  if (ret) *ret = g.heap + g.heapRetOff;
  return FM_OK;
}

// bounded-spin budget for the in-kernel flag waits; FM_P2P_SPIN_LOG2
// shrinks it for the forced-timeout test
static long long p2pSpinBound() {
  // re-read per call: the forced-timeout test shrinks it at runtime
  const char* e = getenv("FM_P2P_SPIN_LOG2");
  const int lg = e ? atoi(e) : 26;
  return 1ll << (lg < 4 ? 4 : (lg > 40 ? 40 : lg));
}

// a previously-completed k_await_flags timeout poisons the transport:
// surface it at the next P2P entry (no sync needed - the flag is
// host-mapped) and definitively via fm_p2p_error_check below
static int p2pPoisonCheck() {
  if (g.hP2pErr && *reinterpret_cast<volatile uint32_t*>(g.hP2pErr)) {
    setErr("p2p exchange timed out (k_await_flags gave up; output poisoned)");
    return FM_ERR_HIP;
  }
  return FM_OK;
}

int fm_p2p_error_check(void* stream) {
  if (!g.heap) { setErr("fm_heap_init/connect first"); return FM_ERR_STATE; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  FM_HIP_CHECK(hipStreamSynchronize(st));
  const int rc = p2pPoisonCheck();
  if (rc != FM_OK && g.hP2pErr) *g.hP2pErr = 0;  // ack: allow retry
  return rc;
}

int fm_dispatch_p2p(void* stream, const void* x) {
  if (!g.heap) { setErr("fm_heap_init/connect first"); return FM_ERR_STATE; }
  int prc = p2pPoisonCheck();
  if (prc != FM_OK) return prc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  g.seq += 1;
  FM_HIP_CHECK(hipMemsetAsync(g.dArrive, 0, 2 * (size_t)g.E * 4, st));
  const int nLx = g.E / g.world;
  dim3 grid(g.EC, g.E);
#define DP2P(T)                                                               \
  hipLaunchKernelGGL(k_dispatch_p2p<T>, grid, dim3(128), 0, st,               \
                     reinterpret_cast<const T*>(x), g.tokenIds, g.eC,         \
                     g.dPeerRecv, g.dPeerDFlag, g.dArrive, g.H, g.EC, g.pEC,  \
                     nLx, g.rank, g.seq)
  if (g.cfg.dtype == 3) DP2P(fp16);
  else if (g.esz == 2) DP2P(bf16);
  else DP2P(float);
#undef DP2P
  FM_HIP_CHECK(hipGetLastError());
  // wait for every source's cells for MY experts
  hipLaunchKernelGGL(
      k_await_flags, dim3(1), dim3(256), 0, st,
      reinterpret_cast<const unsigned long long*>(g.heap + g.heapDFlagOff),
      g.E, g.seq, g.dP2pErr, p2pSpinBound());
  FM_HIP_CHECK(hipGetLastError());
  return FM_OK;
}

int fm_return_p2p(void* stream, const void* ffn_out) {
  if (!g.heap) { setErr("fm_heap_init/connect first"); return FM_ERR_STATE; }
  int prc = p2pPoisonCheck();
  if (prc != FM_OK) return prc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nLx = g.E / g.world;
  dim3 grid(g.EC, g.world * nLx);
#define RP2P(T)                                                               \
  hipLaunchKernelGGL(k_return_p2p<T>, grid, dim3(128), 0, st,                 \
                     reinterpret_cast<const T*>(ffn_out), g.dPeerRet,         \
                     g.dPeerRFlag, g.dArrive + g.E, g.H, g.EC, nLx, g.rank,   \
                     g.seq)
  if (g.cfg.dtype == 3) RP2P(fp16);
  else if (g.esz == 2) RP2P(bf16);
  else RP2P(float);
#undef RP2P
  FM_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(
      k_await_flags, dim3(1), dim3(256), 0, st,
      reinterpret_cast<const unsigned long long*>(g.heap + g.heapRFlagOff),
      g.E, g.seq, g.dP2pErr, p2pSpinBound());
  FM_HIP_CHECK(hipGetLastError());
  return FM_OK;
}

int fm_pack_dispatch(void* stream, const void* x, void* sendbuf) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid(g.EC, g.E);
  if (g.cfg.dtype == 3)
    hipLaunchKernelGGL(k_pack_dispatch<fp16>, grid, dim3(128), 0, st,
                       reinterpret_cast<const fp16*>(x), g.tokenIds, g.eC,
                       reinterpret_cast<fp16*>(sendbuf), g.H, g.EC, g.pEC);
  else if (g.esz == 2)
    hipLaunchKernelGGL(k_pack_dispatch<bf16>, grid, dim3(128), 0, st,
                       reinterpret_cast<const bf16*>(x), g.tokenIds, g.eC,
                       reinterpret_cast<bf16*>(sendbuf), g.H, g.EC, g.pEC);
  else
    hipLaunchKernelGGL(k_pack_dispatch<float>, grid, dim3(128), 0, st,
                       reinterpret_cast<const float*>(x), g.tokenIds, g.eC,
                       reinterpret_cast<float*>(sendbuf), g.H, g.EC, g.pEC);
  FM_HIP_CHECK(hipGetLastError());
  return FM_OK;
}

int fm_combine_padded(void* stream, const void* returned, const void* gate_out,
                      void* moe_out, int64_t S) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  if (S != g.S) { setErr("S mismatch"); return FM_ERR_SHAPE; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid(g.EC, g.E);
  const int tk = g.cfg.expert_top_k;
  if (tk == 1) {
    // k==1: unscaled direct write path via the slot buffer would be
    // redundant; write slots with scale 1 and reduce with the mask
    // (kept mask is exact, so semantics match the reference's
    // CombineMode::single overwrite of a zeroed output)
  }
#define KCP(T)                                                                \
  hipLaunchKernelGGL(k_combine_padded<T>, grid, dim3(256), 0, st,             \
                     reinterpret_cast<const T*>(returned), g.tokenIds, g.eC,  \
                     reinterpret_cast<const T*>(gate_out),                    \
                     reinterpret_cast<T*>(g.cbuf), g.H, g.EC, g.pEC, g.PX, tk)
  if (g.cfg.dtype == 3) KCP(fp16);
  else if (g.esz == 2) KCP(bf16);
  else KCP(float);
#undef KCP
  FM_HIP_CHECK(hipGetLastError());
  if (tk > 1) return launch_cast_combine(st, moe_out);
  // k==1: each token has exactly one slot; reduce with K=1 semantics
  const size_t n = (size_t)g.S * g.H;
  const int blocks = (int)std::min((size_t)4096, (size_t)DIVUP(n, (size_t)256 * 4));
#define CC1(T)                                                                \
  hipLaunchKernelGGL((k_cast_combine<T, 1>), dim3(blocks), dim3(256), 0, st,  \
                     reinterpret_cast<const T*>(g.cbuf), g.kept,              \
                     reinterpret_cast<T*>(moe_out), g.S, g.H)
  if (g.cfg.dtype == 3) CC1(fp16);
  else if (g.esz == 2) CC1(bf16);
  else CC1(float);
#undef CC1
  FM_HIP_CHECK(hipGetLastError());
  return FM_OK;
}

int fm_expert_ffn_segments(void* stream, const void* rows,
                           const void* seg_expert_dev, int32_t n_segs,
                           const void* expert_w, void* out_rows) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  if ((int64_t)n_segs * g.EC > (int64_t)g.nLxAlloc * g.pEC) {
    setErr("segments exceed xM workspace"); return FM_ERR_SHAPE;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (g.cfg.dtype == 5) {
    // MX: quantize the received rows once; the MX GEMM reads x8/scales
    int qrc = launch_quant_mx(st, rows, g.x8, g.xs,
                              (long long)n_segs * g.EC, g.H);
    if (qrc != FM_OK) return qrc;
  }
  GemmArgs up{};
  up.A = (g.cfg.dtype == 5) ? (const void*)g.x8 : rows;
  up.aScales = g.xs;
  up.B = expert_w;
  up.bias = nullptr;
  up.out = g.xM;
  up.tokenIds = nullptr;
  up.eC = nullptr;
  up.strideAExpert = (long long)g.EC * g.H;
  up.strideBExpert = (long long)g.wMats * g.P * g.H;
  up.strideOExpert = (long long)g.EC * g.P;
  up.K = g.H;
  up.N = g.P;
  up.EC = 0;
  up.pEC = 0;
  up.PX = g.PX;
  up.topk = 1;
  up.act = g.cfg.hidden_act;
  up.expertOffset = 0;
  up.nRows = g.EC;
  up.H = g.H;
  up.splitK = 1;
  up.segExpert = reinterpret_cast<const int32_t*>(seg_expert_dev);
  setWeightScaleArgs(up, 0, 0, true);  // indexed by the mapped weight expert
  const bool mxEpiQuant =
      (g.cfg.dtype == 5) && mxWideN(g.EC, g.P, n_segs);
  if (mxEpiQuant) {
    up.out8 = g.xM8;
    up.outScales = g.xMs;
  }
  int rc = launch_group_gemm(st, 0, up, g.EC, n_segs);
  if (rc != FM_OK) return rc;
  if (g.cfg.dtype == 5 && !mxEpiQuant) {
    int qrc = launch_quant_mx(st, g.xM, g.xM8, g.xMs,
                              (long long)n_segs * g.EC, g.P);
    if (qrc != FM_OK) return qrc;
  }
  GemmArgs dn = up;
  dn.out8 = nullptr;
  dn.outScales = nullptr;
  dn.A = (g.cfg.dtype == 5) ? (const void*)g.xM8 : g.xM;
  dn.aScales = g.xMs;
  dn.B = reinterpret_cast<const char*>(expert_w) + (size_t)g.P * g.H * g.wesz;
  dn.out = out_rows;
  dn.strideAExpert = (long long)g.EC * g.P;
  dn.strideOExpert = (long long)g.EC * g.H;
  dn.K = g.P;
  dn.N = g.H;
  setWeightScaleArgs(dn, 1, 0, true);
  return launch_group_gemm(st, 2, dn, g.EC, n_segs);
}

int fm_expert_ffn_grouped(void* stream, const void* rows,
                          const int64_t* offsets, int32_t n_experts,
                          const void* expert_w, const void* b_up,
                          const void* b_dn, void* out_rows) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  for (int le = 0; le < n_experts; ++le) {
    const int64_t n = offsets[le + 1] - offsets[le];
    if (n <= 0) continue;
    const char* r = reinterpret_cast<const char*>(rows) +
                    (size_t)offsets[le] * g.H * g.esz;
    char* o = reinterpret_cast<char*>(out_rows) +
              (size_t)offsets[le] * g.H * g.esz;
    const void* bu = b_up ? reinterpret_cast<const char*>(b_up) +
                                (size_t)le * g.P * g.esz
                          : nullptr;
    const void* bd = b_dn ? reinterpret_cast<const char*>(b_dn) +
                                (size_t)le * g.H * g.esz
                          : nullptr;
    int rc = fm_expert_ffn(stream, r, expert_w, bu, bd, o, n, le);
    if (rc != FM_OK) return rc;
  }
  return FM_OK;
}

int fm_combine(void* stream, const void* rows, const uint32_t* token_idx,
               const float* scale, int64_t n_rows, int32_t zero_first) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (zero_first)
    FM_HIP_CHECK(hipMemsetAsync(g.O32, 0, (size_t)g.S * g.H * sizeof(float), st));
  if (n_rows <= 0) return FM_OK;
  // always accumulate into the fp32 buffer; caller passes scale=1.0 rows
  // for the k==1 unscaled semantics (each token appears at most once)
  if (g.cfg.dtype == 3) {
    hipLaunchKernelGGL((k_combine_rows<fp16, true>), dim3((int)n_rows),
                       dim3(256), 0, st, reinterpret_cast<const fp16*>(rows),
                       token_idx, scale, g.O32, (fp16*)nullptr, g.H);
  } else if (g.esz == 2) {
    hipLaunchKernelGGL((k_combine_rows<bf16, true>), dim3((int)n_rows),
                       dim3(256), 0, st, reinterpret_cast<const bf16*>(rows),
                       token_idx, scale, g.O32, (bf16*)nullptr, g.H);
  } else {
    hipLaunchKernelGGL((k_combine_rows<float, true>), dim3((int)n_rows),
                       dim3(256), 0, st, reinterpret_cast<const float*>(rows),
                       token_idx, scale, g.O32, (float*)nullptr, g.H);
  }
  FM_HIP_CHECK(hipGetLastError());
  return FM_OK;
}

int fm_combine_finalize(void* stream, void* moe_out, int64_t S) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  if (S != g.S) { setErr("S mismatch"); return FM_ERR_SHAPE; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t n = (size_t)g.S * g.H;
  const int blocks = (int)min((size_t)2048, DIVUP(n, (size_t)256 * 8));
  if (g.cfg.dtype == 3)
    hipLaunchKernelGGL(k_cast_out<fp16>, dim3(blocks), dim3(256), 0, st, g.O32,
                       reinterpret_cast<fp16*>(moe_out), n);
  else if (g.esz == 2)
    hipLaunchKernelGGL(k_cast_out<bf16>, dim3(blocks), dim3(256), 0, st, g.O32,
                       reinterpret_cast<bf16*>(moe_out), n);
  else
    hipLaunchKernelGGL(k_cast_out<float>, dim3(blocks), dim3(256), 0, st,
                       g.O32, reinterpret_cast<float*>(moe_out), n);
  FM_HIP_CHECK(hipGetLastError());
  return FM_OK;
}

int fm_export_routing(void* stream, void* routed_dev, void* tps_dev) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_export_routing, dim3(g.E), dim3(256), 0, st,
                     g.tokenIds,
                     (g.lastForwardFused && g.fusedCtl) ? fusedECPtr() : g.eC,
                     reinterpret_cast<uint32_t*>(routed_dev),
                     reinterpret_cast<uint32_t*>(tps_dev), g.E, g.EC, g.pEC);
  FM_HIP_CHECK(hipGetLastError());
  return FM_OK;
}

int fm_read_aux_loss(void* stream, float* gML, float* gMeC) {
  if (!g.initialized) { setErr("not initialized"); return FM_ERR_STATE; }
  if (!g.cfg.is_training) { setErr("aux loss requires is_training=1"); return FM_ERR_STATE; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  FM_HIP_CHECK(hipMemcpyAsync(gML, g.gML, (size_t)g.E * sizeof(float),
                              hipMemcpyDeviceToHost, st));
  FM_HIP_CHECK(hipMemcpyAsync(gMeC, g.gMeC, (size_t)g.E * sizeof(float),
                              hipMemcpyDeviceToHost, st));
  FM_HIP_CHECK(hipStreamSynchronize(st));
  return FM_OK;
}

// ---------------------------------------------------------------------------
// Device task-queue primitive (round-2 groundwork; reference semantics:
// subscriber::start polling + scheduler::start matching,
// os/subscriber.cuh:333-451 / os/scheduler.cuh:296-441). A seqlock MPMC
// ring of 128-B task descriptors with generation tags:
//   producer of slot s (gen g = s/ring):  wait seq[pos]==2g  -> write desc
//     -> release-store seq[pos]=2g+1
//   consumer of slot s:                   wait seq[pos]==2g+1 -> read desc
//     -> release-store seq[pos]=2g+2
// Device-scope atomics (single GPU); bounded spins so a logic bug aborts
// instead of hanging the box. The fused persistent kernel
// will drive expert tiles through this queue; here it is validated by a
// standalone probe (fm_debug_taskq): P producer blocks enqueue nTasks
// descriptors, C consumer blocks drain them, each task consumed exactly
// once (checksum + count verified on the host).
// ---------------------------------------------------------------------------

struct __align__(128) FmTask {
  uint32_t kind, payload, slot, gen;
  uint32_t pad[28];
};

__global__ void k_taskq_probe(FmTask* ring, uint32_t* seq, uint32_t ringSz,
                              uint32_t nTasks, uint64_t* tail,
                              uint64_t* claim, uint32_t* sum,
                              uint32_t* consumed, uint32_t* errors) {
  const bool producer = (blockIdx.x & 1) == 0;
  if (threadIdx.x != 0) return;  // block-level protocol; lane 0 drives
  if (producer) {
    while (true) {
      const uint64_t s = atomicAdd(reinterpret_cast<unsigned long long*>(tail),
                                   1ull);
      if (s >= nTasks) break;
      const uint32_t pos = (uint32_t)(s % ringSz);
      const uint32_t gen = (uint32_t)(s / ringSz);
      uint32_t spins = 0;
      while (__hip_atomic_load(seq + pos, __ATOMIC_ACQUIRE,
                               __HIP_MEMORY_SCOPE_AGENT) != 2u * gen) {
        if (++spins > (1u << 26)) { atomicAdd(errors, 1u); return; }
        __builtin_amdgcn_s_sleep(2);
      }
      ring[pos].kind = 1;
      ring[pos].payload = (uint32_t)(s * 2654435761u);  // checksum source
      ring[pos].slot = (uint32_t)s;
      ring[pos].gen = gen;
      __hip_atomic_store(seq + pos, 2u * gen + 1u, __ATOMIC_RELEASE,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
  } else {
    while (true) {
      const uint64_t s = atomicAdd(reinterpret_cast<unsigned long long*>(claim),
                                   1ull);
      if (s >= nTasks) break;
      const uint32_t pos = (uint32_t)(s % ringSz);
      const uint32_t gen = (uint32_t)(s / ringSz);
      uint32_t spins = 0;
      while (__hip_atomic_load(seq + pos, __ATOMIC_ACQUIRE,
                               __HIP_MEMORY_SCOPE_AGENT) != 2u * gen + 1u) {
        if (++spins > (1u << 26)) { atomicAdd(errors, 1u); return; }
        __builtin_amdgcn_s_sleep(2);
      }
      const FmTask t = ring[pos];
      if (t.slot != (uint32_t)s || t.gen != gen) atomicAdd(errors, 1u);
      atomicAdd(sum, t.payload);
      atomicAdd(consumed, 1u);
      __hip_atomic_store(seq + pos, 2u * gen + 2u, __ATOMIC_RELEASE,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// test-only probe (see k_mfma_probe)
int fm_debug_fp8cvt(void* stream, const void* in256, void* out256_f32) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_fp8cvt_probe, dim3(1), dim3(32), 0, st,
                     reinterpret_cast<const uint32_t*>(in256),
                     reinterpret_cast<float*>(out256_f32));
  FM_HIP_CHECK(hipGetLastError());
  return FM_OK;
}

int fm_debug_taskq(void* stream, int ring_sz, long long n_tasks,
                   int blocks, uint32_t* out_sum, uint32_t* out_consumed,
                   uint32_t* out_errors) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  FmTask* ring = nullptr;
  uint32_t* seq = nullptr;
  uint64_t* ctrs = nullptr;  // tail, claim
  uint32_t* acc = nullptr;   // sum, consumed, errors
  FM_HIP_CHECK(hipMalloc(&ring, (size_t)ring_sz * sizeof(FmTask)));
  FM_HIP_CHECK(hipMalloc(&seq, (size_t)ring_sz * sizeof(uint32_t)));
  FM_HIP_CHECK(hipMalloc(&ctrs, 2 * sizeof(uint64_t)));
  FM_HIP_CHECK(hipMalloc(&acc, 3 * sizeof(uint32_t)));
  FM_HIP_CHECK(hipMemsetAsync(seq, 0, (size_t)ring_sz * sizeof(uint32_t), st));
  FM_HIP_CHECK(hipMemsetAsync(ctrs, 0, 2 * sizeof(uint64_t), st));
  FM_HIP_CHECK(hipMemsetAsync(acc, 0, 3 * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_taskq_probe, dim3(blocks), dim3(64), 0, st, ring, seq,
                     (uint32_t)ring_sz, (uint32_t)n_tasks, ctrs, ctrs + 1,
                     acc, acc + 1, acc + 2);
  FM_HIP_CHECK(hipGetLastError());
  uint32_t h[3];
  FM_HIP_CHECK(hipMemcpyAsync(h, acc, sizeof(h), hipMemcpyDeviceToHost, st));
  FM_HIP_CHECK(hipStreamSynchronize(st));
  if (out_sum) *out_sum = h[0];
  if (out_consumed) *out_consumed = h[1];
  if (out_errors) *out_errors = h[2];
  (void)hipFree(ring); (void)hipFree(seq); (void)hipFree(ctrs); (void)hipFree(acc);
  return FM_OK;
}

int fm_debug_mx_mfma(void* stream, const void* A, const void* B,
                     const void* sa, const void* sb, void* D, int opsel) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define MXP(O)                                                                  hipLaunchKernelGGL(k_mx_mfma_probe<O>, dim3(1), dim3(64), 0, st,                                 reinterpret_cast<const uint8_t*>(A),                                          reinterpret_cast<const uint8_t*>(B),                                          reinterpret_cast<const uint8_t*>(sa),                                         reinterpret_cast<const uint8_t*>(sb),                                         reinterpret_cast<float*>(D))
  switch (opsel) {
    case 1: MXP(1); break;
    case 2: MXP(2); break;
    case 3: MXP(3); break;
    default: MXP(0); break;
  }
#undef MXP
  FM_HIP_CHECK(hipGetLastError());
  return FM_OK;
}

int fm_debug_mfma(void* stream, const void* A, const void* B, void* D) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_mfma_probe, dim3(1), dim3(64), 0, st,
                     reinterpret_cast<const bf16*>(A),
                     reinterpret_cast<const bf16*>(B),
                     reinterpret_cast<float*>(D));
  FM_HIP_CHECK(hipGetLastError());
  return FM_OK;
}

#ifdef FM_GEMM_STAMPS
// measurement build only: copy the phase stamps out (dst holds
// 4 x 512 x 4 x 4 uint64) and zero them for the next forward
int fm_debug_gemm_stamps(void* dst) {
  FM_HIP_CHECK(hipDeviceSynchronize());
  FM_HIP_CHECK(hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_gemmStamps),
                                   sizeof(g_gemmStamps)));
  void* p = nullptr;
  FM_HIP_CHECK(hipGetSymbolAddress(&p, HIP_SYMBOL(g_gemmStamps)));
  FM_HIP_CHECK(hipMemset(p, 0, sizeof(g_gemmStamps)));
  return FM_OK;
}
// the same for the gate / combine entry-exit stamps (dst holds
// 2 x 4096 x 2 uint64)
int fm_debug_aux_stamps(void* dst) {
  FM_HIP_CHECK(hipDeviceSynchronize());
  FM_HIP_CHECK(hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_auxStamps),
                                   sizeof(g_auxStamps)));
  void* p = nullptr;
  FM_HIP_CHECK(hipGetSymbolAddress(&p, HIP_SYMBOL(g_auxStamps)));
  FM_HIP_CHECK(hipMemset(p, 0, sizeof(g_auxStamps)));
  return FM_OK;
}
#endif
}  // extern "C"
