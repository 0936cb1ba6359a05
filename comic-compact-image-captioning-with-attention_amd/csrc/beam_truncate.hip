// Top-k and nucleus (top-p) truncation of the sampled beam step (extends rnn_decoder_beam_search, common/ops_rnn.py:49-112):
// which candidates a live slot may draw from, as ban bits.  Runs after beam_bans.hip has built the constraints' mask (if
// any) and before the sampled step (beam_step.hip, the Samples policy under Bans) ranks.
//
// The rule (the contract: include/comic_hip.h, comic_beam_truncation), for a live slot (b, w) at step t:
//   lp[v]  the policy's step log-probability: step_lp of beam_policy.h, the code the beam step itself ranks by
//   a[v] = lp[v] * inv_temp in fp32, inv_temp = 1.0f / temperature formed once on the host (what the Samples policy uses)
//   A      the allowed set: the tokens whose ban bit is clear (no constraints: all V tokens)
//   top-k  (top_k >= 1; 0 = off) K = the top_k largest a over A, equal values resolved by lowest v; top_k >= |A|: K = A
//   top-p  (0 < top_p < 1; >= 1 = off) m = max_K a, e[v] = exp(a[v] - m), Z = sum_K e; tau = the largest value among a[K]
//          with sum_{u in K, a[u] >= tau} e[u] >= top_p * Z (a product, never a division); v in K is kept iff a[v] >= tau:
//          every candidate tied at the boundary value is kept.  The nucleus is taken on the distribution renormalised over
//          K: temperature -> top-k -> top-p.
//   mask   every token of a live row that is not kept gets its ban bit set; bits already set stay set; the best allowed
//          candidate is always kept; a row whose m is not finite (all banned, or a NaN) is left as it came; a finished row
//          is not touched (_mask_probs makes it emit <EOS> as ever).
// Nothing else changes: the sampled step ranks lp[v] * inv_temp + g over the survivors, and the state / scores stay the
// model's own unperturbed, untempered, UNTRUNCATED log p(caption | image).
//
// One workgroup of 1024 threads per row (b, w); W <= 64, V <= 65 536.
//   keys     a[v] is formed ONCE per row (an expf / logf per member and candidate) and kept as its order-preserving
//            uint32 image -- key 0 marks "not a candidate" (banned, or dropped by top-k) -- in LDS when the row fits
//            (V <= 32 768: the word vocabulary's 25 599 keys are 100 KB of the 160 KB, one workgroup per CU), else in a
//            scratch row of the caller's workspace.  d[v] = key_max - key[v] is the distance below the best candidate.
//   select   both stages are ONE digit-wise descent over d, most significant used digit first, 8 bits a pass: the
//            smallest d* whose cumulative weight, from the best candidate down, reaches a target.  Top-k weighs every
//            candidate 1 and targets top_k (the k-th key; a prefix count in v order over the candidates equal to it gives
//            the lowest-v tie rule).  Top-p weighs a candidate by its mass and targets top_p * Z.
//   sums     every histogram is an array of 64-bit INTEGERS in LDS.  A mass enters as the fixed-point number
//            floor(e[v] * 2^40) (e <= 1; a row's truncation error is below V * 2^-40 of Z >= 1, four orders under the
//            fp32 rounding of e itself), so every sum is exact and cannot depend on the order in which waves arrive:
//            two runs give the same bits.  No float is ever accumulated across threads.  Z is the total of the first
//            pass's histogram; the comparison is S >= ceil(double(top_p) * double(Z)).
//   output   a wave forms 64 bits at a time by ballot and ONE lane stores each 32-bit word with a plain vector store:
//            every word of a row has one owner, no atomics touch the mask.  Without constraints every word of every row
//            is written (a finished row as zeros); bits at positions >= V are zero.
#include <math.h>

#include "beam_policy.h"

namespace {

constexpr int kTruncThreads = 1024, kTruncWaves = kTruncThreads / 64;
constexpr int kTruncLdsKeys = 32768;       // keys of a row kept in LDS: 128 KB beside ~9 KB of static LDS
constexpr int kTruncMaxV = 65536;
constexpr float kMassScale = 1099511627776.0f;   // 2^40

typedef unsigned long long u64;

// order-preserving image of a float: a < b  <=>  key(a) < key(b) (negative NaNs lowest, positive NaNs highest); never 0
// for a number
__device__ __forceinline__ uint32_t trunc_key(float a) {
  const uint32_t u = __float_as_uint(a);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float trunc_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// 1024-thread reductions of a float: DPP inside a wave, the 16 wave results through LDS, combined by every thread in wave
// order -- the same bits in every thread and every run.  `sh` [16]; two barriers, so `sh` may be reused at once.
template <bool kMax>
__device__ __forceinline__ float trunc_block_reduce(float v, float* sh) {
  v = kMax ? wave_max(v) : wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
#pragma unroll
  for (int k = 1; k < kTruncWaves; ++k) r = kMax ? fmaxf(r, sh[k]) : r + sh[k];
  __syncthreads();
  return r;
}

struct TruncShared {
  u64 hist[256];
  u64 digit, below;            // a descent pass's result: the digit taken, the weight strictly better than it
  float red[kTruncWaves];
  uint32_t key_hi, key_lo;     // the largest / smallest key of a candidate
  int n_cand, nan;
  int wave_ties[kTruncWaves];
};

// The smallest d* = key_hi - key over the row's candidates whose cumulative weight sum_{d <= d*} reaches the target;
// *below = the weight of d < d*.  kMass: a candidate weighs floor(exp(a - m) * 2^40) and the target is
// ceil(top_p * total), total being the first pass's histogram; else it weighs 1 and the target is `count`.  max_d bounds
// d over the candidates.  Every thread of the workgroup calls it and gets the same result.
template <bool kMass>
__device__ uint32_t trunc_descend(const uint32_t* row, int V, uint32_t key_hi, uint32_t max_d, float m, u64 count, float top_p,
                                  TruncShared& s, u64* below) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int nbits = max_d ? 32 - __clz(max_d) : 0;
  int width = min(8, nbits), shift = nbits - width;
  uint32_t prefix = 0;                     // the digits taken so far: d* >> (shift + width)
  u64 acc = 0, target = count;             // (target: wave 0's copy is the one that counts)
  bool first = true;
  while (true) {
    if (tid < 256) s.hist[tid] = 0;
    __syncthreads();
    const uint32_t dmask = (1u << width) - 1u;
    for (int v = tid; v < V; v += kTruncThreads) {
      const uint32_t key = row[v];
      if (!key) continue;
      const uint32_t d = key_hi - key;
      const uint32_t upper = shift + width >= 32 ? 0u : d >> (shift + width);
      if (upper != prefix) continue;
      const u64 wgt = kMass ? (u64)(expf(trunc_unkey(key) - m) * kMassScale) : (u64)1;
      atomicAdd(&s.hist[(d >> shift) & dmask], wgt);
    }
    __syncthreads();
    if (tid < 64) {                        // wave 0: lane l owns bins 4 l .. 4 l + 3
      const u64 h0 = s.hist[4 * lane], h1 = s.hist[4 * lane + 1], h2 = s.hist[4 * lane + 2], h3 = s.hist[4 * lane + 3];
      const u64 mine = (h0 + h1) + (h2 + h3);
      u64 inc = mine;                      // inclusive scan over the lanes
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const u64 up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
      }
      if (kMass && first) {
        const u64 total = __shfl(inc, 63, 64);
        const double want = ceil((double)top_p * (double)total);
        target = want < 1.0 ? (u64)1 : (u64)want;
      }
      const u64 ex = acc + (inc - mine);
      const u64 crossed = __ballot(ex + mine >= target);
      const int owner = crossed ? __ffsll((long long)crossed) - 1 : 63;
      if (lane == owner) {
        u64 c = ex;
        int j = 0;
        if (c + h0 >= target) j = 0;
        else if (c + h0 + h1 >= target) { j = 1; c += h0; }
        else if (c + h0 + h1 + h2 >= target) { j = 2; c += h0 + h1; }
        else { j = 3; c += h0 + h1 + h2; }
        s.digit = (u64)(4 * lane + j);
        s.below = c;
      }
    }
    __syncthreads();
    prefix = (prefix << width) | (uint32_t)s.digit;         // (width <= 8)
    acc = s.below;
    first = false;
    if (shift == 0) break;
    width = min(8, shift);
    shift -= width;
  }
  __syncthreads();                         // (s.digit / s.below may be rewritten by the next descent)
  *below = acc;
  return prefix;
}

template <bool kLds>
__global__ __launch_bounds__(kTruncThreads) void beam_truncate_kernel(const float* __restrict__ logits, Ensemble pol,
                                                                      const int32_t* __restrict__ finished,
                                                                      uint32_t* __restrict__ bits, int words, int B, int W,
                                                                      int V, float inv_temp, int top_k, float top_p,
                                                                      int has_bans, uint32_t* __restrict__ scratch,
                                                                      const int32_t* __restrict__ stop, int stop_t) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_keys[];
  __shared__ Ensemble::Rows rows;
  __shared__ TruncShared s;
  if (comic_stopped(stop, stop_t)) return;
  const int r = blockIdx.x, b = r / W, w = r - b * W;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t* out = bits + (size_t)r * words;
  uint32_t* row;
  if constexpr (kLds) row = s_keys;
  else row = scratch + (size_t)r * V;
  // a row the stages leave alone: untouched under constraints, else all zeros (the incoming content is not a mask then)
  auto leave = [&]() {
    if (!has_bans)
      for (int k = tid; k < words; k += kTruncThreads) out[k] = 0u;
  };
  if (finished[r] != 0) {                  // (uniform over the workgroup)
    leave();
    return;
  }
  if (tid == 0) {
    s.key_hi = 0u;
    s.key_lo = 0xffffffffu;
    s.n_cand = 0;
    s.nan = 0;
  }
  pol.begin(rows);
  // the row's log-softmax constants per member that counts, as the one-workgroup beam step forms them
  const size_t mstride = (size_t)B * W * V;
  const float* lg = logits + (size_t)b * W * V;
  for (int m = 0; m < pol.members(); ++m) {
    if (!pol.live(rows, m)) continue;
    const float* x = lg + m * mstride + (size_t)w * V;
    float mx = -INFINITY;
    for (int v = tid; v < V; v += kTruncThreads) mx = fmaxf(mx, x[v]);
    mx = trunc_block_reduce<true>(mx, s.red);
    float sum = 0.f;
    for (int v = tid; v < V; v += kTruncThreads) sum += expf(x[v] - mx);
    sum = trunc_block_reduce<false>(sum, s.red);
    if (tid == 0) {
      rows.mx[m * 64 + w] = mx;
      rows.logsum[m * 64 + w] = logf(sum);
    }
  }
  __syncthreads();
  // the keys of a[v], once per row
  {
    uint32_t hi = 0u, lo = 0xffffffffu;
    int cnt = 0, nan = 0;
    for (int v = tid; v < V; v += kTruncThreads) {
      uint32_t key = 0u;
      if (!(has_bans && ((out[v >> 5] >> (v & 31)) & 1u))) {
        const float a = pol.step_lp(lg, mstride, w * V + v, w, rows) * inv_temp;
        nan |= (a != a) ? 1 : 0;
        key = trunc_key(a);
        hi = max(hi, key);
        lo = min(lo, key);
        ++cnt;
      }
      row[v] = key;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      hi = max(hi, (uint32_t)__shfl_xor((int)hi, o, 64));
      lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, 64));
      cnt += __shfl_xor(cnt, o, 64);
      nan |= __shfl_xor(nan, o, 64);
    }
    if (lane == 0) {                       // integer atomics: exact, whatever the order
      atomicMax(&s.key_hi, hi);
      atomicMin(&s.key_lo, lo);
      atomicAdd(&s.n_cand, cnt);
      atomicOr(&s.nan, nan);
    }
  }
  __syncthreads();
  const uint32_t key_hi = s.key_hi;
  uint32_t key_lo = s.key_lo;
  const int n_cand = s.n_cand;
  const float m = trunc_unkey(key_hi);
  if (n_cand == 0 || s.nan || !(fabsf(m) <= FLT_MAX)) {      // all banned, a NaN, or a best candidate that is not finite
    leave();
    return;
  }
  // ---- top-k: the k-th key, then the lowest v among the candidates equal to it ---------------------------------------
  if (top_k > 0 && top_k < n_cand) {
    u64 better = 0;
    const uint32_t dk = trunc_descend<false>(row, V, key_hi, key_hi - key_lo, m, (u64)top_k, 1.f, s, &better);
    const int need = top_k - (int)better;                     // of the candidates at distance dk, in v order
    const int per = (V + kTruncThreads - 1) / kTruncThreads, v0 = min(V, tid * per), v1 = min(V, v0 + per);
    int ties = 0;
    for (int v = v0; v < v1; ++v) {
      const uint32_t key = row[v];
      ties += (key && key_hi - key == dk) ? 1 : 0;
    }
    int inc = ties;                                           // exclusive prefix over the threads, i.e. over v
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    if (lane == 63) s.wave_ties[wave] = inc;
    __syncthreads();
    int rank = inc - ties;
    for (int k = 0; k < wave; ++k) rank += s.wave_ties[k];
    for (int v = v0; v < v1; ++v) {
      const uint32_t key = row[v];
      if (!key) continue;
      const uint32_t d = key_hi - key;
      if (d > dk || (d == dk && rank++ >= need)) row[v] = 0u;
    }
    key_lo = key_hi - dk;
    __syncthreads();
  }
  // ---- top-p over what is left: the distance of tau below the best candidate ---------------------------------------------
  uint32_t dp = key_hi - key_lo;                              // (off: every candidate is kept)
  if (top_p < 1.f) {
    u64 unused = 0;
    dp = trunc_descend<true>(row, V, key_hi, key_hi - key_lo, m, 0, top_p, s, &unused);
  }
  // ---- the mask: 64 candidates per wave and round, one lane stores each word ---------------------------------------------
  for (int base = wave * 64; base < words * 32; base += kTruncThreads) {
    const int v = base + lane;
    bool drop = false;
    if (v < V) {
      const uint32_t key = row[v];
      drop = !key || key_hi - key > dp;
    }
    const u64 bal = __ballot(drop);
    const int word = (base >> 5) + lane;
    if (lane < 2 && word < words) out[word] = (uint32_t)(bal >> (32 * lane));
  }
}

int64_t truncate_scratch_bytes(int B, int W, int V) { return V > kTruncLdsKeys ? (int64_t)B * W * V * 4 : 0; }

}  // namespace

// executor-internal (decoder_exec.hip checks a loop's truncation once, in front of its first launch).  `whole`: the rules
// of a whole decode -- the raw operator also takes a top_k that reaches V, which changes nothing.
int comic_beam_truncation_check(const comic_beam_truncation* tr, const char* who, int V, bool whole) {
  COMIC_REQUIRE(tr, "%s: null truncation", who);
  COMIC_REQUIRE(tr->top_k >= 0, "%s: top_k %d is negative", who, tr->top_k);
  COMIC_REQUIRE(tr->top_p > 0.f, "%s: top_p must be > 0 and not NaN", who);
  COMIC_REQUIRE(tr->top_k >= 1 || tr->top_p < 1.f, "%s: truncation with top_k 0 and top_p >= 1: both stages are off", who);
  COMIC_REQUIRE(V > 0 && V <= kTruncMaxV, "%s: truncation: vocabulary V = %d outside [1,%d]", who, V, kTruncMaxV);
  if (whole)
    COMIC_REQUIRE(tr->top_k < V || tr->top_p < 1.f, "%s: top_k %d reaches V = %d and top_p >= 1: the truncation does nothing",
                  who, tr->top_k, V);
  return 0;
}

extern "C" int64_t comic_beam_truncate_workspace(int n_models, int B, int W, int V) {
  if (n_models < 1 || n_models > kEnsMax || B <= 0 || W <= 0 || W > 64 || V <= 0 || V > kTruncMaxV) return -1;
  return truncate_scratch_bytes(B, W, V);
}

extern "C" int comic_beam_truncate(const float* logits, const float* weights, int n_models, const int32_t* finished,
                                   uint32_t* bits, int words, int B, int W, int V, float temperature,
                                   const comic_beam_truncation* truncation, int has_bans, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  const char* who = "beam_truncate";
  COMIC_REQUIRE(logits && finished && bits, "%s: null pointer", who);
  if (int rc = comic_beam_truncation_check(truncation, who, V, false)) return rc;
  COMIC_REQUIRE(B > 0 && W >= 1 && W <= 64 && (long)B * W * V < (1L << 31), "%s: bad shape", who);
  COMIC_REQUIRE(words == (V + 31) / 32, "%s: %d mask words for a vocabulary of %d", who, words, V);
  COMIC_REQUIRE(temperature > 0.f && temperature <= FLT_MAX && 1.0f / temperature <= FLT_MAX,
                "%s: temperature must be finite and > 0 with a finite reciprocal", who);
  COMIC_REQUIRE((long)n_models * B <= 65535, "%s: members * batch too large", who);
  Ensemble pol{};
  if (int rc = comic_ensemble_policy(who, weights, n_models, &pol)) return rc;
  const int64_t need = truncate_scratch_bytes(B, W, V);
  COMIC_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "%s: workspace too small (%lld bytes needed)", who,
                (long long)need);
  hipStream_t st = (hipStream_t)stream;
  const float inv_temp = 1.0f / temperature;
  if (need == 0) {
    const int lds = V * 4;
    static PerDeviceOnce attr_once__;
    bool& attr_set = attr_once__.slot();   // hipFuncSetAttribute holds per device
    if (!attr_set) {
      if (hipFuncSetAttribute((const void*)beam_truncate_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              kTruncLdsKeys * 4) != hipSuccess) {
        comic_set_error("%s: cannot reserve %d bytes of LDS", who, kTruncLdsKeys * 4);
        return 1;
      }
      attr_set = true;
    }
    hipLaunchKernelGGL(beam_truncate_kernel<true>, dim3(B * W), dim3(kTruncThreads), lds, st, logits, pol, finished, bits,
                       words, B, W, V, inv_temp, truncation->top_k, truncation->top_p, has_bans ? 1 : 0, (uint32_t*)nullptr,
                       g_comic_stop.p, g_comic_stop.t);
  } else {
    hipLaunchKernelGGL(beam_truncate_kernel<false>, dim3(B * W), dim3(kTruncThreads), 0, st, logits, pol, finished, bits,
                       words, B, W, V, inv_temp, truncation->top_k, truncation->top_p, has_bans ? 1 : 0,
                       (uint32_t*)workspace, g_comic_stop.p, g_comic_stop.t);
  }
  COMIC_LAUNCH_CHECK("beam_truncate");
  return 0;
}
