// Consensus (minimum-Bayes-risk) selection among the W decoded candidates of an image: every candidate's mean CIDEr-D
// similarity to its siblings, on token ids, in one launch.  No counterpart in the reference decode (common/ops_rnn.py);
// the similarity is the one of common/scst/cider_ruotianluo/pyciderevalcap/ciderD/ciderD_scorer.py:52-222.
//
// The contract (units, weights, similarity, utility, table, limits) is include/comic_hip.h, comic_caption_consensus.
//
// One workgroup of 1024 threads per image; everything but the idf table lives in LDS:
//   rows   the image's [T][W] slice of the ids, copied as it lies in memory (lanes run over w: coalesced, no conflicts).
//          It is dead once the keys exist and shares its bytes with `vec`.
//   keys   uint64 [4 * Ucap][W], Ucap = min(64, T / stride): entry (k * Ucap + i, w) is the key of candidate w's n-gram of
//          order k + 1 that starts at unit i -- splitmix64 chained over its tokens, the hash the idf table is built with --
//          or 0 where the candidate has no such n-gram.  N-GRAM EQUALITY IS DECIDED ON THESE 64-BIT KEYS.
//   vec    double, same shape: tf * g at the FIRST occurrence of an n-gram in its candidate; the keys of the later
//          occurrences are zeroed, so an entry with a non-zero key is a distinct n-gram.  g comes from one probe sequence in
//          global memory per distinct n-gram of a candidate, never one per pair.
//   norm   double [4][W]; len, U int [W]; pi double [W]; sim double [W][W].
// Phases, a barrier between each: copy -> first <EOS> and U per candidate -> keys -> tf and first occurrences -> g and vec
// -> norms (one lane per (k, w), ascending unit) and pi (one lane) -> the W * (W - 1) ordered pairs, one lane each, summed
// over h's n-grams in first-occurrence order, r's searched linearly -> utilities (one lane per w, ascending sibling) ->
// best (one lane).  All arithmetic is float64 and every sum has one owner and one order: two runs give the same bits, and
// nothing depends on how workgroups interleave.  Plain vector stores only.
//
// Where the time goes: the pair phase, W * (W - 1) lanes each comparing up to 4 * U * U keys in LDS; at 32 candidates of
// 20 units that is ~1 600 compares a lane, four per LDS load.  The launch is latency-bound, not throughput-bound, and its
// time hardly depends on W: every pair has a lane of its own.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/comic_hip.h"
#include "common.h"
#include "ngram_dev.h"

namespace {

constexpr int kConsThreads = 1024;
constexpr int kConsMaxW = 32;        // candidates of an image
constexpr int kConsMaxU = 64;        // units of a candidate (the header states this bound)
constexpr int kConsMaxStride = 8;    // tokens of a unit: the rows of W * T ids must fit the bytes of `vec`
constexpr int kConsOrders = 4;       // n-gram orders 1..4
constexpr int kConsBlock = 4;        // n-grams of h compared per pass over a sibling's

typedef unsigned long long u64;

struct ConsFixed {                   // the part of the LDS whose size does not depend on T
  double sim[kConsMaxW * kConsMaxW];
  double norm[kConsOrders * kConsMaxW];
  double pi[kConsMaxW];
  int U[kConsMaxW];
  int len[kConsMaxW];
};

__host__ __device__ inline int cons_ucap(int T, int stride) {
  const int u = T / stride;
  return u < 1 ? 1 : (u > kConsMaxU ? kConsMaxU : u);
}
// bytes of `keys`, and of `vec` (which also holds the rows before the keys exist)
__host__ __device__ inline size_t cons_key_bytes(int W, int T, int stride) {
  return (size_t)kConsOrders * cons_ucap(T, stride) * W * sizeof(u64);
}
__host__ __device__ inline size_t cons_vec_bytes(int W, int T, int stride) {
  const size_t v = cons_key_bytes(W, T, stride), r = (((size_t)W * T * sizeof(int32_t)) + 7) & ~(size_t)7;
  return v > r ? v : r;
}
inline size_t cons_lds_bytes(int W, int T, int stride) {
  return sizeof(ConsFixed) + cons_key_bytes(W, T, stride) + cons_vec_bytes(W, T, stride);
}

__global__ __launch_bounds__(kConsThreads) void consensus_kernel(
    const int32_t* __restrict__ ids, int T, int B, int W, int end_id, int stride, const float* __restrict__ log_probs,
    const u64* __restrict__ tab_keys, const double* __restrict__ tab_g, long long tab_cap, double log_ref_len,
    double two_sigma2, double* __restrict__ utility, int32_t* __restrict__ best) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  ConsFixed& S = *reinterpret_cast<ConsFixed*>(lds_raw);
  u64* keys = reinterpret_cast<u64*>(lds_raw + sizeof(ConsFixed));
  double* vec = reinterpret_cast<double*>(lds_raw + sizeof(ConsFixed) + cons_key_bytes(W, T, stride));
  int32_t* rows = reinterpret_cast<int32_t*>(vec);           // [T][W]; dead after the key phase
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Ucap = cons_ucap(T, stride), P = kConsOrders * Ucap;

  // ---- the image's rows, as they lie in memory
  for (int e = tid; e < T * W; e += kConsThreads) {
    const int t = e / W, w = e - t * W;
    rows[e] = ids[((size_t)t * B + b) * W + w];
  }
  __syncthreads();
  // ---- first <EOS>, units, length (the bigram count: the host scorer's own rule)
  if (tid < W) {
    int L = T;
    for (int t = 0; t < T; ++t)
      if (rows[t * W + tid] == end_id) {
        L = t;
        break;
      }
    int U = L / stride;
    if (U > kConsMaxU) U = kConsMaxU;                        // (the entry refuses T > 64 * stride: never taken)
    S.U[tid] = U;
    S.len[tid] = U > 1 ? U - 1 : 0;
  }
  __syncthreads();
  // ---- keys: entry (p, w), p = k * Ucap + i
  for (int e = tid; e < P * W; e += kConsThreads) {
    const int p = e / W, w = e - p * W, k = p / Ucap, i = p - k * Ucap;
    u64 key = 0;
    if (i + k + 1 <= S.U[w]) {
      key = ngram_key(rows + (size_t)i * stride * W + w, (k + 1) * stride, W);
    }
    keys[e] = key;
  }
  __syncthreads();                                           // rows are dead from here: vec takes their bytes
  // ---- term frequency; a later occurrence is marked with -1
  for (int e = tid; e < P * W; e += kConsThreads) {
    const int p = e / W, w = e - p * W, k = p / Ucap, i = p - k * Ucap;
    const u64 key = keys[e];
    double tf = 0.0;
    if (key) tf = ngram_tf(keys + (size_t)k * Ucap * W + w, S.U[w] - k, W, i);
    vec[e] = tf;
  }
  __syncthreads();
  // ---- g of every distinct n-gram (one probe sequence each), vec = tf * g; later occurrences lose their key
  for (int e = tid; e < P * W; e += kConsThreads) {
    const u64 key = keys[e];
    if (!key) continue;
    const double tf = vec[e];
    if (tf < 0.0) {
      keys[e] = 0;
      continue;
    }
    const double g = ngram_idf(tab_keys, tab_g, tab_cap, log_ref_len, key);
    vec[e] = tf * g;
  }
  __syncthreads();
  // ---- norms, one lane per (k, w) in ascending unit order; the slot weights, one lane
  if (tid < kConsOrders * W) {
    const int k = tid / W, w = tid - k * W, n = S.U[w] - k;
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
      const int e = (k * Ucap + i) * W + w;
      if (keys[e]) s += vec[e] * vec[e];
    }
    S.norm[tid] = sqrt(s);
  } else if (tid == kConsThreads - 1) {
    if (!log_probs) {
      for (int w = 0; w < W; ++w) S.pi[w] = 1.0;
    } else {
      const float* lp = log_probs + (size_t)b * W;
      double m = -INFINITY, z = 0.0;
      for (int w = 0; w < W; ++w) m = fmax(m, (double)lp[w]);
      for (int w = 0; w < W; ++w) {
        const double x = (double)lp[w];
        const double v = (m > -INFINITY && x > -INFINITY) ? exp(x - m) : 0.0;
        S.pi[w] = v;
        z += v;
      }
      for (int w = 0; w < W; ++w) S.pi[w] = z > 0.0 ? S.pi[w] / z : 0.0;
    }
  }
  __syncthreads();
  // ---- the ordered pairs: candidate h against sibling r, one lane each
  for (int e = tid; e < W * W; e += kConsThreads) {
    const int h = e / W, r = e - h * W;
    if (h == r) {
      S.sim[e] = 0.0;
      continue;
    }
    const double d = (double)(S.len[h] - S.len[r]);
    const double pen = exp(-(d * d) / two_sigma2);
    double total = 0.0;
    for (int k = 0; k < kConsOrders; ++k) {
      const int nh = S.U[h] - k, nr = S.U[r] - k;
      double val = 0.0;
      // kConsBlock n-grams of h at a time against one pass over r's: the loads of a pass do not depend on one another, so
      // they overlap; a serial search with an early exit is bound by one LDS latency per compare.  A key occurs once in r
      // (later occurrences lost theirs), and the products are added in h's order.
      for (int i0 = 0; i0 < nh; i0 += kConsBlock) {
        u64 kh[kConsBlock];
        int hit[kConsBlock];
#pragma unroll
        for (int a = 0; a < kConsBlock; ++a) {
          kh[a] = i0 + a < nh ? keys[(k * Ucap + i0 + a) * W + h] : 0;
          hit[a] = -1;
        }
#pragma unroll 4
        for (int q = 0; q < nr; ++q) {
          const u64 kr = keys[(k * Ucap + q) * W + r];
#pragma unroll
          for (int a = 0; a < kConsBlock; ++a)
            if (kr == kh[a]) hit[a] = q;
        }
#pragma unroll
        for (int a = 0; a < kConsBlock; ++a)
          if (kh[a] && hit[a] >= 0) {
            const double vr = vec[(k * Ucap + hit[a]) * W + r];
            val += fmin(vec[(k * Ucap + i0 + a) * W + h], vr) * vr;
          }
      }
      const double nn_h = S.norm[k * W + h], nn_r = S.norm[k * W + r];
      if (nn_h != 0.0 && nn_r != 0.0) val /= nn_h * nn_r;
      total += val * pen;
    }
    S.sim[e] = total / kConsOrders * 10.0;
  }
  __syncthreads();
  // ---- utilities: a sequential sum over the siblings in ascending slot order
  if (tid < W) {
    double num = 0.0, den = 0.0;
    for (int j = 0; j < W; ++j)
      if (j != tid) {
        num += S.pi[j] * S.sim[tid * W + j];
        den += S.pi[j];
      }
    const double u = !(S.pi[tid] > 0.0) ? -INFINITY : (den > 0.0 ? num / den : 0.0);
    utility[(size_t)b * W + tid] = u;
    S.sim[tid * W + tid] = u;                                // the diagonal is free: the hand-over to the last lane
  }
  __syncthreads();
  if (tid == 0) {
    int at = 0;
    double top = -INFINITY;
    for (int w = 0; w < W; ++w) {
      const double u = S.sim[w * W + w];
      if (S.pi[w] > 0.0 && u > top) {
        top = u;
        at = w;
      }
    }
    best[b] = at;
  }
}

int consensus_check(const char* who, int T, int B, int W, int stride) {
  COMIC_REQUIRE(B >= 1 && T >= 1, "%s: B = %d and T = %d must be >= 1", who, B, T);
  COMIC_REQUIRE(W >= 1 && W <= kConsMaxW, "%s: W = %d candidates, 1 to %d are supported", who, W, kConsMaxW);
  COMIC_REQUIRE(stride >= 1 && stride <= kConsMaxStride, "%s: stride = %d, 1 to %d are supported", who, stride,
                kConsMaxStride);
  COMIC_REQUIRE(T <= kConsMaxU * stride, "%s: T = %d exceeds %d units of %d tokens", who, T, kConsMaxU, stride);
  return 0;
}

}  // namespace

extern "C" int64_t comic_caption_consensus_workspace(int B, int W, int T, int stride) {
  if (consensus_check("caption_consensus_workspace", T, B, W, stride)) return -1;
  return 0;                        // every intermediate lives in LDS
}

extern "C" int comic_caption_consensus(const int32_t* ids_tbw, int T, int B, int W, int end_id, int stride,
                                       const float* log_probs_or_null, int weights_mode,
                                       const uint64_t* table_keys_or_null, const double* table_g, int64_t table_cap,
                                       double log_ref_len, double sigma, double* utility_bw, int32_t* best_b,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "caption_consensus";
  if (int rc = consensus_check(who, T, B, W, stride)) return rc;
  COMIC_REQUIRE(ids_tbw && utility_bw && best_b, "%s: ids, utility and best must not be NULL", who);
  COMIC_REQUIRE(weights_mode == COMIC_CONSENSUS_UNIFORM || weights_mode == COMIC_CONSENSUS_POSTERIOR,
                "%s: weights_mode %d is neither uniform (0) nor posterior (1)", who, weights_mode);
  COMIC_REQUIRE(weights_mode == COMIC_CONSENSUS_UNIFORM || log_probs_or_null,
                "%s: the posterior weights need the log-probabilities", who);
  COMIC_REQUIRE(sigma > 0.0 && std::isfinite(sigma), "%s: sigma must be finite and > 0, got %g", who, sigma);
  if (table_keys_or_null) {
    COMIC_REQUIRE(table_g, "%s: a table of keys without its g values", who);
    COMIC_REQUIRE(table_cap >= 1 && (table_cap & (table_cap - 1)) == 0, "%s: table_cap = %lld is no power of two", who,
                  (long long)table_cap);
    COMIC_REQUIRE(std::isfinite(log_ref_len), "%s: log_ref_len must be finite", who);
  }
  (void)workspace;
  (void)workspace_bytes;
  const size_t lds = cons_lds_bytes(W, T, stride);
  COMIC_REQUIRE(lds <= 160u * 1024u, "%s: %zu bytes of LDS exceed a workgroup's 160 KiB", who, lds);
  static PerDeviceOnce attr_once__;
  bool& attr_set = attr_once__.slot();   // hipFuncSetAttribute holds per device
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)consensus_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
        hipSuccess) {
      comic_set_error("%s: cannot reserve the LDS", who);
      return 1;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL(consensus_kernel, dim3(B), dim3(kConsThreads), lds, (hipStream_t)stream, ids_tbw, T, B, W, end_id,
                     stride, weights_mode == COMIC_CONSENSUS_POSTERIOR ? log_probs_or_null : (const float*)nullptr,
                     (const u64*)table_keys_or_null, table_g, (long long)table_cap, log_ref_len,
                     2.0 * sigma * sigma, utility_bw, best_b);
  COMIC_LAUNCH_CHECK(who);
  return 0;
}
