// The SCST reward on the device: CIDEr-D and per-sentence BLEU-1..4 of every rollout of an image against the image's
// reference captions, the baseline and the advantage, in one launch; and the loss coefficients the update reads, formed
// from that advantage without a host round trip.  The host scorer it restates is common/scst/scorers.py:43-171
// (captionScorer.get_hypo_scores) over ciderD_scorer.py:52-222 and bleu_scorer.py:23-263.
//
// The contract (canonical words, references, metrics, baselines, limits) is include/comic_hip.h, comic_scst_reward.
//
// One workgroup of 1024 threads per image, modelled on consensus.hip; everything but the idf table lives in LDS.  The
// captions of an image are its W rollouts, the optional baseline row, then its R references: N = W' + R captions of at
// most Ucap words each, caption c's entries contiguous:
//   rows   the image's [T][W] slice of the ids, the [T0] baseline row and the [R][Lr] references, copied as they lie in
//          memory (coalesced; no lane walks global memory word by word); dead once the words exist, and shares its
//          bytes with `vec`.
//   words  int32 [N][Ucap]: the canonical word ids (the ids ops.id_to_caption(skip_unmapped=True) turns into text).
//   keys   uint64 [N][4][Ucap]: the key of the n-gram of order k + 1 that starts at word i, 0 where there is none.
//          N-GRAM EQUALITY IS DECIDED ON THESE 64-BIT KEYS (ngram_dev.h, shared with consensus.hip).
//   vec    double, same shape: tf * g at the first occurrence of an n-gram; later occurrences lose their key.
//   tfc    uint8, same shape: tf at the first occurrence (BLEU's clipped counts).
// Phases, a barrier between each: copy (the last wave reduces the baseline row's executed steps from the first-<EOS>
// positions) -> canonical words (one lane per caption, one pass) -> keys -> tf, and g and vec at first occurrences (one
// idf probe per distinct n-gram) -> later occurrences lose their keys, norms (one lane per (caption, order)) -> CIDEr-D,
// one lane per (rollout, reference, order), beside BLEU's clipped matches, one lane per n-gram of a rollout, added to
// their (rollout, order) count by an LDS integer add -> the metrics, one lane per (rollout, BLEU order) and per rollout's CIDEr-D ->
// reward, baseline and advantage, one lane per rollout.  All floating-point arithmetic is float64 and every such sum has one owner and one
// order: two runs give the same bits.  Plain vector stores only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/comic_hip.h"
#include "common.h"
#include "ngram_dev.h"

namespace {

constexpr int kRewThreads = 1024;
constexpr int kRewMaxW = 32;         // rollouts of an image
constexpr int kRewMaxWt = kRewMaxW + 1;   // ... and the baseline row
constexpr int kRewMaxR = 8;          // references of an image
constexpr int kRewMaxU = 64;         // words of a caption
constexpr int kRewMaxWordLen = 8;    // digits of a radix word: the rows of W' * T ids must fit the bytes of `vec`
constexpr int kRewOrders = 4;
constexpr int kRewBlock = 4;         // n-grams of a rollout compared per pass over a reference's
constexpr size_t kRewLdsMax = 160u * 1024u;

typedef ngram_u64 u64;

struct RewFixed {                    // the part of the LDS whose size does not depend on the geometry
  double pair[kRewMaxWt * kRewMaxR * kRewOrders];   // CIDEr-D: val_k of (rollout, reference)
  double norm[(kRewMaxWt + kRewMaxR) * kRewOrders];
  double cider[kRewMaxWt];
  double bleu[kRewMaxWt * kRewOrders];
  int correct[kRewMaxWt * kRewOrders];              // BLEU: clipped matches of (rollout, order)
  int nw[kRewMaxWt + kRewMaxR];                     // words of a caption
  int t_exec;                                       // rows of the baseline row that were executed
};

struct RewArgs {
  const int32_t* ids;                // [T, B, W]
  const int32_t* base_ids;           // [T0, B] or NULL
  const int32_t* base_first_eos;     // [B] or NULL
  const int32_t* refs;               // [B, R, Lr]
  const int32_t* n_refs;             // [B]
  const u64* tab_keys;
  const double* tab_g;
  long long tab_cap;
  double log_ref_len, two_sigma2, w_cider, w_bleu[4];
  double *cider, *bleu, *reward, *baseline;
  float* advantage;
  int T, B, W, T0, R, Lr, Ucap;
  int radix, end_id, base, word_len, vocab, mode;
};

inline int rew_ucap(int T, int T0, int word_len, int Lr) {
  int u = (T + word_len - 1) / word_len;
  const int u0 = (T0 + word_len - 1) / word_len;
  if (u0 > u) u = u0;
  if (Lr > u) u = Lr;
  return u < 1 ? 1 : u;
}
__host__ __device__ inline size_t rew_key_bytes(int N, int Ucap) { return (size_t)N * kRewOrders * Ucap * sizeof(u64); }
inline size_t rew_vec_bytes(int N, int Ucap, int W, int T, int T0) {
  const size_t v = rew_key_bytes(N, Ucap);
  const size_t r = ((((size_t)W * T + T0 + (size_t)kRewMaxR * Ucap) * sizeof(int32_t)) + 7) & ~(size_t)7;   // rows, row, references
  return v > r ? v : r;
}
inline size_t rew_lds_bytes(int W, int Wt, int R, int Ucap, int T, int T0) {
  const int N = Wt + R;
  return sizeof(RewFixed) + rew_key_bytes(N, Ucap) + rew_vec_bytes(N, Ucap, W, T, T0) +
         (size_t)N * Ucap * sizeof(int32_t) + (size_t)N * kRewOrders * Ucap;
}

// kRewBlock n-grams of caption h (keys kh) against one pass over the nr keys of another caption: the loads of a pass do
// not depend on one another, so they overlap.  A key occurs once in a caption (later occurrences lost theirs).
__device__ __forceinline__ void rew_find(const u64* kr_, int nr, const u64 (&kh)[kRewBlock], int (&hit)[kRewBlock]) {
#pragma unroll
  for (int a = 0; a < kRewBlock; ++a) hit[a] = -1;
#pragma unroll 4
  for (int q = 0; q < nr; ++q) {
    const u64 kr = kr_[q];
#pragma unroll
    for (int a = 0; a < kRewBlock; ++a)
      if (kr == kh[a]) hit[a] = q;
  }
}

__global__ __launch_bounds__(kRewThreads) void scst_reward_kernel(const RewArgs A, size_t vec_bytes) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int T = A.T, B = A.B, W = A.W, T0 = A.T0, R = A.R, Lr = A.Lr, Ucap = A.Ucap;
  const int Wt = W + (A.base_ids ? 1 : 0), N = Wt + R, P = kRewOrders * Ucap;
  RewFixed& S = *reinterpret_cast<RewFixed*>(lds_raw);
  u64* keys = reinterpret_cast<u64*>(lds_raw + sizeof(RewFixed));
  double* vec = reinterpret_cast<double*>(lds_raw + sizeof(RewFixed) + rew_key_bytes(N, Ucap));
  int32_t* words = reinterpret_cast<int32_t*>(lds_raw + sizeof(RewFixed) + rew_key_bytes(N, Ucap) + vec_bytes);
  unsigned char* tfc = reinterpret_cast<unsigned char*>(words + (size_t)N * Ucap);
  int32_t* rows = reinterpret_cast<int32_t*>(vec);           // [T][W] then [T0]; dead after the word phase
  const int b = blockIdx.x, tid = threadIdx.x;
  int Rn = A.n_refs[b];
  Rn = Rn < 0 ? 0 : (Rn > R ? R : Rn);
  const bool do_cider = A.w_cider > 0.0;
  const bool do_bleu = fmax(fmax(A.w_bleu[0], A.w_bleu[1]), fmax(A.w_bleu[2], A.w_bleu[3])) > 0.0;

  // ---- the image's rows and references, as they lie in memory; the last wave finds the baseline row's executed steps
  int32_t* raw_refs = rows + T * W + T0;                     // [Rn][Lr]
  for (int e = tid; e < T * W; e += kRewThreads) {
    const int t = e / W, w = e - t * W;
    rows[e] = A.ids[((size_t)t * B + b) * W + w];
  }
  if (A.base_ids)
    for (int t = tid; t < T0; t += kRewThreads) rows[T * W + t] = A.base_ids[(size_t)t * B + b];
  for (int e = tid; e < Rn * Lr; e += kRewThreads) raw_refs[e] = A.refs[(size_t)b * R * Lr + e];
  if (tid >= kRewThreads - 64) {
    const int j = tid - (kRewThreads - 64);
    int m = T0 - 1;
    if (A.base_first_eos) {                                  // the loop that wrote the row ended when every image had its <EOS>
      m = -1;
      for (int x = j; x < B; x += 64) {
        const int f = A.base_first_eos[x];
        m = f > m ? f : m;
      }
      for (int o = 32; o; o >>= 1) {
        const int f = __shfl_xor(m, o, 64);
        m = f > m ? f : m;
      }
    }
    if (j == 0) S.t_exec = m + 1 < 0 ? 0 : (m + 1 > T0 ? T0 : m + 1);
  }
  if (tid < kRewMaxWt * kRewOrders) S.correct[tid] = 0;
  __syncthreads();
  // ---- canonical words, one lane per caption
  if (tid < N) {
    int32_t* out = words + (size_t)tid * Ucap;
    int n = 0;
    if (tid >= Wt) {                                         // a reference: its word ids up to the padding
      const int r = tid - Wt;
      if (r < Rn) {
        const int32_t* src = raw_refs + r * Lr;
        for (int i = 0; i < Lr; ++i) {
          const int32_t v = src[i];
          if (v >= 0 && n < Ucap) out[n++] = v;
        }
      }
    } else {
      const int32_t* src = tid < W ? rows + tid : rows + T * W;
      const int step = tid < W ? W : 1, len = tid < W ? T : S.t_exec;
      if (!A.radix) {                                        // tokens >= 0 and != <EOS>, wherever they stand
        for (int t = 0; t < len; ++t) {
          const int32_t v = src[t * step];
          if (v >= 0 && v != A.end_id && v < A.vocab && n < Ucap) out[n++] = v;
        }
      } else {
        // one pass: a full group is emitted when the next digit arrives or the row ends; `prev` is the open group less
        // its last digit, which is what remains of a short last group once ONE trailing digit is dropped
        long long acc = 0, prev = 0;
        int in_group = 0;
        for (int t = 0; t < len; ++t) {
          const int32_t v = src[t * step];
          if (v < 0 || v >= A.base) continue;
          if (in_group == A.word_len) {
            if (acc < A.vocab && n < Ucap) out[n++] = (int32_t)acc;
            acc = 0;
            in_group = 0;
          }
          prev = acc;
          acc = acc * A.base + v;
          if (acc > A.vocab) acc = A.vocab;                  // beyond the table it stays beyond it: no overflow at any word_len
          ++in_group;
        }
        if (in_group == A.word_len) prev = acc;              // a multiple of the word length: nothing is dropped
        if ((in_group == A.word_len || in_group > 1) && prev < A.vocab && n < Ucap) out[n++] = (int32_t)prev;
      }
    }
    S.nw[tid] = n;
  }
  __syncthreads();                                           // rows are dead from here: vec takes their bytes
  // ---- keys: entry e = (c * 4 + k) * Ucap + i
  for (int e = tid; e < N * P; e += kRewThreads) {
    const int c = e / P, p = e - c * P, k = p / Ucap, i = p - k * Ucap;
    keys[e] = i + k + 1 <= S.nw[c] ? ngram_key(words + (size_t)c * Ucap + i, k + 1, 1) : 0;
  }
  __syncthreads();
  // ---- term frequency, and at an n-gram's first occurrence its g (one probe sequence each): vec = tf * g, tfc = tf;
  //      tfc = 0 marks a later occurrence
  for (int e = tid; e < N * P; e += kRewThreads) {
    const int c = e / P, p = e - c * P, k = p / Ucap, i = p - k * Ucap;
    const u64 key = keys[e];
    double v = 0.0;
    int tf = 0;
    if (key) {
      const double f = ngram_tf(keys + (size_t)(c * kRewOrders + k) * Ucap, S.nw[c] - k, 1, i);
      if (f > 0.0) {
        tf = (int)f;
        v = f * ngram_idf(A.tab_keys, A.tab_g, A.tab_cap, A.log_ref_len, key);
      }
    }
    vec[e] = v;
    tfc[e] = (unsigned char)tf;
  }
  __syncthreads();
  // ---- later occurrences lose their key; norms, one lane per (caption, order) in ascending word order (they read tfc
  //      and vec, not the keys)
  for (int e = tid; e < N * P; e += kRewThreads)
    if (!tfc[e]) keys[e] = 0;
  if (tid < N * kRewOrders) {
    const int c = tid / kRewOrders, k = tid - c * kRewOrders, n = S.nw[c] - k;
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
      const int e = tid * Ucap + i;
      if (tfc[e]) s += vec[e] * vec[e];
    }
    S.norm[tid] = sqrt(s);
  }
  __syncthreads();
  // ---- CIDEr-D: one lane per (rollout h, reference r, order k), summed over h's n-grams in order of first occurrence;
  //      BLEU: one lane per n-gram (h, k, i): its count clipped by the maximum over the references, added to the
  //      (h, k) total in LDS -- integers, so the order of the additions does not show
  const int n_pair = do_cider ? Wt * Rn * kRewOrders : 0, n_gram = do_bleu ? Wt * P : 0;
  for (int x = tid; x < n_pair + n_gram; x += kRewThreads) {
    if (x < n_pair) {
      const int hr = x / kRewOrders, k = x - hr * kRewOrders, h = hr / Rn, r = hr - h * Rn, cr = Wt + r;
      const int lh = S.nw[h] > 1 ? S.nw[h] - 1 : 0, lr = S.nw[cr] > 1 ? S.nw[cr] - 1 : 0;   // the bigram counts
      const double d = (double)(lh - lr);
      const double pen = exp(-(d * d) / A.two_sigma2);
      const int nh = S.nw[h] - k, nr = S.nw[cr] - k;
      const int eh = (h * kRewOrders + k) * Ucap, er = (cr * kRewOrders + k) * Ucap;
      double val = 0.0;
      for (int i0 = 0; i0 < nh; i0 += kRewBlock) {
        u64 kh[kRewBlock];
        int hit[kRewBlock];
#pragma unroll
        for (int a = 0; a < kRewBlock; ++a) kh[a] = i0 + a < nh ? keys[eh + i0 + a] : 0;
        rew_find(keys + er, nr, kh, hit);
#pragma unroll
        for (int a = 0; a < kRewBlock; ++a)
          if (kh[a] && hit[a] >= 0) {
            const double vr = vec[er + hit[a]];
            val += fmin(vec[eh + i0 + a], vr) * vr;
          }
      }
      const double nn_h = S.norm[h * kRewOrders + k], nn_r = S.norm[cr * kRewOrders + k];
      if (nn_h != 0.0 && nn_r != 0.0) val /= nn_h * nn_r;
      S.pair[(h * kRewMaxR + r) * kRewOrders + k] = val * pen;
    } else {
      const int e = x - n_pair, hk = e / Ucap, k = hk & (kRewOrders - 1);
      const u64 key = keys[e];                               // (rollouts come first: e is the entry's index)
      if (!key) continue;
      int mx = 0;
      for (int r = 0; r < Rn; ++r) {
        const int er = ((Wt + r) * kRewOrders + k) * Ucap, nr = S.nw[Wt + r] - k;
        int hit = -1;
#pragma unroll 4
        for (int q = 0; q < nr; ++q)
          if (keys[er + q] == key) hit = q;
        if (hit >= 0) {
          const int c = tfc[er + hit];
          mx = c > mx ? c : mx;
        }
      }
      const int c = tfc[e];
      if (mx) atomicAdd(&S.correct[hk], c < mx ? c : mx);
    }
  }
  __syncthreads();
  // ---- the metrics: BLEU-k of rollout h in lane (h, k) -- each lane forms the running product up to its order and its
  //      own pow -- and CIDEr-D of rollout h in lane Wt * 4 + h
  if (tid < Wt * kRewOrders) {
    const int h = tid / kRewOrders, k = tid - h * kRewOrders;
    double v = 0.0;
    if (do_bleu) {
      const double small = 1e-9, tiny = 1e-15;
      const int testlen = S.nw[h];
      int reflen = 0, best = 0x7fffffff;
      for (int r = 0; r < Rn; ++r) {                         // 'closest', ties to the shorter
        const int l = S.nw[Wt + r], d = l > testlen ? l - testlen : testlen - l;
        if (d < best || (d == best && l < reflen)) {
          best = d;
          reflen = l;
        }
      }
      double run = 1.0;
      for (int j = 0; j <= k; ++j) {
        const int guess = testlen - j > 0 ? testlen - j : 0;
        run *= ((double)S.correct[h * kRewOrders + j] + tiny) / ((double)guess + small);
      }
      v = pow(run, 1.0 / (k + 1));
      const double ratio = ((double)testlen + tiny) / ((double)reflen + small);
      if (ratio < 1.0) v *= exp(1.0 - 1.0 / ratio);
    }
    S.bleu[tid] = v;
  } else if (tid < Wt * (kRewOrders + 1)) {
    const int h = tid - Wt * kRewOrders;
    double cider = 0.0;
    if (do_cider) {
      double sum = 0.0;
      for (int k = 0; k < kRewOrders; ++k) {
        double s = 0.0;
        for (int r = 0; r < Rn; ++r) s += S.pair[(h * kRewMaxR + r) * kRewOrders + k];
        sum += s;
      }
      cider = sum / kRewOrders / (double)Rn * 10.0;
    }
    S.cider[h] = cider;
  }
  __syncthreads();
  // ---- the reward, the baseline and the advantage, one lane per rollout; every lane forms the totals it needs itself, in
  //      the one order (cider, then BLEU-1..4), so they are the same bits in every lane.  The advantage is
  //      hypothesis-major (row w * B + b)
  if (tid < Wt) {
    auto total = [&](int h) {
      double t = 0.0;
      if (do_cider) t += S.cider[h] * A.w_cider;
      if (do_bleu)
        for (int k = 0; k < kRewOrders; ++k) t += S.bleu[h * kRewOrders + k] * A.w_bleu[k];
      return t;
    };
    const double mine = total(tid);
    const size_t o = (size_t)b * Wt + tid;
    A.cider[o] = S.cider[tid];
    for (int k = 0; k < kRewOrders; ++k) A.bleu[o * kRewOrders + k] = S.bleu[tid * kRewOrders + k];
    A.reward[o] = mine;
    if (tid < W) {
      double base = 0.0;
      if (A.mode == COMIC_SCST_BASELINE_ROW) {
        base = total(W);
      } else if (A.mode == COMIC_SCST_BASELINE_LEAVE_ONE_OUT) {
        double s = 0.0;
        for (int j = 0; j < W; ++j)
          if (j != tid) s += total(j);
        base = s / (double)(W - 1);
      }
      A.baseline[(size_t)b * W + tid] = base;
      A.advantage[(size_t)tid * B + b] = (float)(mine - base);
    }
  }
}

// The loss coefficients of the SCST update from the staged mask and the advantage: the float32 operations of
// Decoder.train_step's host formula, correctly rounded and uncontracted.  One lane per row.
__global__ void scst_coefficients_kernel(const float* __restrict__ wmask, const float* __restrict__ adv, int rows, int T,
                                         float* __restrict__ coef, float* __restrict__ rs) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const float* m = wmask + (size_t)r * T;
  float sum = 0.0f;
  for (int t = 0; t < T; ++t) sum = __fadd_rn(sum, m[t]);   // a 0/1 mask: exact in any order
  const float den = __fadd_rn(sum, 1e-12f);
  const float rb = __fdiv_rn(adv[r], (float)rows);
  const float scale = __fdiv_rn(rb, den);
  for (int t = 0; t < T; ++t) {
    coef[(size_t)r * T + t] = __fmul_rn(__fdiv_rn(m[t], den), rb);
    rs[(size_t)r * T + t] = scale;
  }
}

int reward_check(const char* who, int B, int W, int has_row, int T, int T0, int word_len, int R, int Lr) {
  COMIC_REQUIRE(B >= 1 && T >= 1, "%s: B = %d and T = %d must be >= 1", who, B, T);
  COMIC_REQUIRE(W >= 1 && W <= kRewMaxW, "%s: W = %d rollouts, 1 to %d are supported", who, W, kRewMaxW);
  COMIC_REQUIRE(R >= 1 && R <= kRewMaxR, "%s: R = %d references, 1 to %d are supported", who, R, kRewMaxR);
  COMIC_REQUIRE(word_len >= 1 && word_len <= kRewMaxWordLen, "%s: word_len = %d, 1 to %d are supported", who, word_len,
                kRewMaxWordLen);
  COMIC_REQUIRE(Lr >= 1 && Lr <= kRewMaxU, "%s: Lr = %d reference words, 1 to %d are supported", who, Lr, kRewMaxU);
  COMIC_REQUIRE(T <= kRewMaxU * word_len, "%s: T = %d exceeds %d words of %d tokens", who, T, kRewMaxU, word_len);
  COMIC_REQUIRE(has_row ? (T0 >= 1 && T0 <= kRewMaxU * word_len) : T0 == 0,
                "%s: T0 = %d: 1 to %d with a baseline row, 0 without", who, T0, kRewMaxU * word_len);
  const size_t lds = rew_lds_bytes(W, W + (has_row ? 1 : 0), R, rew_ucap(T, T0, word_len, Lr), T, T0);
  COMIC_REQUIRE(lds <= kRewLdsMax, "%s: %zu bytes of LDS exceed a workgroup's 160 KiB", who, lds);
  return 0;
}

}  // namespace

extern "C" int64_t comic_scst_reward_workspace(int B, int W, int has_baseline_row, int T, int T0, int word_len, int R,
                                               int Lr) {
  if (reward_check("scst_reward_workspace", B, W, has_baseline_row, T, T0, word_len, R, Lr)) return -1;
  return (int64_t)rew_lds_bytes(W, W + (has_baseline_row ? 1 : 0), R, rew_ucap(T, T0, word_len, Lr), T, T0);
}

extern "C" int comic_scst_reward(const int32_t* ids_tbw, int T, int B, int W, const int32_t* baseline_ids_t0b_or_null,
                                 int T0, const int32_t* baseline_first_eos_b_or_null, int token_mode, int end_id, int radix_base, int word_len, int vocab,
                                 const int32_t* refs_brl, const int32_t* n_refs_b, int R, int Lr,
                                 const uint64_t* table_keys_or_null, const double* table_g, int64_t table_cap,
                                 double log_ref_len, double sigma, double w_cider, const double* w_bleu4,
                                 int baseline_mode, double* cider_bw, double* bleu_bw4, double* reward_bw,
                                 double* baseline_bw, float* advantage_wb, void* stream) {
  const char* who = "scst_reward";
  const int has_row = baseline_ids_t0b_or_null != nullptr;
  COMIC_REQUIRE(token_mode == COMIC_SCST_TOKENS_WORD || token_mode == COMIC_SCST_TOKENS_RADIX,
                "%s: token_mode %d is neither word (0) nor radix (1)", who, token_mode);
  if (token_mode == COMIC_SCST_TOKENS_WORD)
    COMIC_REQUIRE(word_len == 1, "%s: word tokens have word_len 1, got %d", who, word_len);
  else
    COMIC_REQUIRE(radix_base >= 2, "%s: radix_base = %d must be >= 2", who, radix_base);
  if (int rc = reward_check(who, B, W, has_row, T, has_row ? T0 : 0, word_len, R, Lr)) return rc;
  COMIC_REQUIRE(ids_tbw && refs_brl && n_refs_b && w_bleu4, "%s: ids, refs, n_refs and w_bleu must not be NULL", who);
  COMIC_REQUIRE(cider_bw && bleu_bw4 && reward_bw && baseline_bw && advantage_wb, "%s: no output may be NULL", who);
  COMIC_REQUIRE(vocab >= 1, "%s: vocab = %d must be >= 1", who, vocab);
  COMIC_REQUIRE(baseline_mode == COMIC_SCST_BASELINE_NONE || baseline_mode == COMIC_SCST_BASELINE_ROW ||
                    baseline_mode == COMIC_SCST_BASELINE_LEAVE_ONE_OUT,
                "%s: baseline_mode %d is none of NONE (0), ROW (1), LEAVE_ONE_OUT (2)", who, baseline_mode);
  COMIC_REQUIRE(baseline_mode != COMIC_SCST_BASELINE_ROW || has_row, "%s: the ROW baseline needs the baseline ids", who);
  COMIC_REQUIRE(baseline_mode != COMIC_SCST_BASELINE_LEAVE_ONE_OUT || W >= 2,
                "%s: the LEAVE_ONE_OUT baseline needs W >= 2, got %d", who, W);
  COMIC_REQUIRE(sigma > 0.0 && std::isfinite(sigma), "%s: sigma must be finite and > 0, got %g", who, sigma);
  COMIC_REQUIRE(std::isfinite(w_cider) && std::isfinite(w_bleu4[0]) && std::isfinite(w_bleu4[1]) &&
                    std::isfinite(w_bleu4[2]) && std::isfinite(w_bleu4[3]), "%s: the weights must be finite", who);
  if (table_keys_or_null) {
    COMIC_REQUIRE(table_g, "%s: a table of keys without its g values", who);
    COMIC_REQUIRE(table_cap >= 1 && (table_cap & (table_cap - 1)) == 0, "%s: table_cap = %lld is no power of two", who,
                  (long long)table_cap);
    COMIC_REQUIRE(std::isfinite(log_ref_len), "%s: log_ref_len must be finite", who);
  }
  RewArgs a;
  a.ids = ids_tbw;
  a.base_ids = baseline_ids_t0b_or_null;
  a.base_first_eos = has_row ? baseline_first_eos_b_or_null : nullptr;
  a.refs = refs_brl;
  a.n_refs = n_refs_b;
  a.tab_keys = (const u64*)table_keys_or_null;
  a.tab_g = table_g;
  a.tab_cap = (long long)table_cap;
  a.log_ref_len = log_ref_len;
  a.two_sigma2 = 2.0 * sigma * sigma;
  a.w_cider = w_cider;
  for (int k = 0; k < 4; ++k) a.w_bleu[k] = w_bleu4[k];
  a.cider = cider_bw;
  a.bleu = bleu_bw4;
  a.reward = reward_bw;
  a.baseline = baseline_bw;
  a.advantage = advantage_wb;
  a.T = T;
  a.B = B;
  a.W = W;
  a.T0 = has_row ? T0 : 0;
  a.R = R;
  a.Lr = Lr;
  a.Ucap = rew_ucap(T, a.T0, word_len, Lr);
  a.radix = token_mode == COMIC_SCST_TOKENS_RADIX;
  a.end_id = end_id;
  a.base = radix_base;
  a.word_len = word_len;
  a.vocab = vocab;
  a.mode = baseline_mode;
  const int Wt = W + has_row;
  const size_t lds = rew_lds_bytes(W, Wt, R, a.Ucap, T, a.T0);
  static PerDeviceOnce attr_once__;
  bool& attr_set = attr_once__.slot();   // hipFuncSetAttribute holds per device
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)scst_reward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kRewLdsMax) != hipSuccess) {
      comic_set_error("%s: cannot reserve the LDS", who);
      return 1;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL(scst_reward_kernel, dim3(B), dim3(kRewThreads), lds, (hipStream_t)stream, a,
                     rew_vec_bytes(Wt + R, a.Ucap, W, T, a.T0));
  COMIC_LAUNCH_CHECK(who);
  return 0;
}

extern "C" int comic_scst_coefficients(const float* wmask_rt, const float* advantage_r, int rows, int T, float* coef_rt,
                                       float* row_scale_rt, void* stream) {
  const char* who = "scst_coefficients";
  COMIC_REQUIRE(rows >= 1 && T >= 1, "%s: rows = %d and T = %d must be >= 1", who, rows, T);
  COMIC_REQUIRE(wmask_rt && advantage_r && coef_rt && row_scale_rt, "%s: no pointer may be NULL", who);
  hipLaunchKernelGGL(scst_coefficients_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, wmask_rt,
                     advantage_r, rows, T, coef_rt, row_scale_rt);
  COMIC_LAUNCH_CHECK(who);
  return 0;
}
