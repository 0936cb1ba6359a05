// Beam search with required words (Anderson et al. 2017; the bank form of Post & Vilar 2018; extends
// rnn_decoder_beam_search, common/ops_rnn.py:49-112): the per-step bookkeeping that the banked step consults (beam_step.hip,
// beam_step_banks_kernel), and the initial state.  The rule is stated at comic_beam_required in include/comic_hip.h.
//
// Row r = (b, w) of step t is the beam that step t - 1 wrote at slot w; its history h[0 .. t-1] is kept exactly as
// beam_bans.hip keeps it (hist[2][R][max_steps], step t reads (t - 1) & 1 and writes t & 1).  When the decode has
// constraints too, beam_bans.hip advances the ONE pair of buffers and this kernel only reads: it forms the row's tokens from
// the sources of that copy (the parent's row of the other buffer, then the last word), so it does not matter which of the
// two launches of a step runs first.
//
// With req[b] = C words of S tokens (-1 rows: padding), L = t and k = L mod S, a row has
//   m        the number of words q that are padding or have an aligned full match h[i .. i+S-1], i % S == 0, i + S <= L
//   base     S * m: where every token without a special leads
//   special  per unmet word q whose first k tokens are the tail h[L-k .. L-1]: the token req[b][q][k], which leads to
//            S * m + k + 1 when k + 1 < S and else to S * (m + gain), gain = the unmet words that token completes
// One workgroup per row; the matches are found by all threads, the table row is written by one.
#include "common.h"

namespace {

constexpr int kReqWords = 4, kReqStride = 4;

__global__ __launch_bounds__(256) void beam_required_kernel(const int32_t* __restrict__ prev_words,
                                                            const int32_t* __restrict__ prev_parents,
                                                            const int32_t* __restrict__ req, int32_t* __restrict__ hist,
                                                            int32_t* __restrict__ base, int32_t* __restrict__ special, int C,
                                                            int S, int t, int R, int W, int V, int max_steps, int write_hist,
                                                            const int32_t* __restrict__ stop, int stop_t) {
  __shared__ int s_req[kReqWords * kReqStride];
  __shared__ int s_met[kReqWords];
  if (comic_stopped(stop, stop_t)) return;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int b = r / W;
  if (tid < C * S) s_req[tid] = req[(size_t)b * C * S + tid];
  __syncthreads();
  if (tid < kReqWords) s_met[tid] = (tid < C && s_req[tid * S] < 0) ? 1 : 0;       // a padding row counts as met
  // the row's history: the parent's row of the other buffer, then the word of the step before
  const int L = t;
  const int32_t* src = nullptr;
  int last = 0;
  if (L > 0) {
    const int parent = min(max(prev_parents[r], 0), W - 1);
    last = min(max(prev_words[r], 0), V - 1);
    src = hist + ((size_t)((t - 1) & 1) * R + (size_t)b * W + parent) * max_steps;
    if (write_hist) {
      int32_t* dst = hist + ((size_t)(t & 1) * R + r) * max_steps;
      for (int j = tid; j < L; j += 256) dst[j] = j < L - 1 ? src[j] : last;
    }
  }
  auto tok = [&](int j) { return j < L - 1 ? min(max(src[j], 0), V - 1) : last; };
  __syncthreads();
  // aligned full matches: window i = S * j
  for (int i = tid * S; i + S <= L; i += 256 * S)
    for (int q = 0; q < C; ++q) {
      if (s_req[q * S] < 0) continue;
      bool same = true;
      for (int k = 0; k < S && same; ++k) same = tok(i + k) == s_req[q * S + k];
      if (same) s_met[q] = 1;                         // (every writer stores the same value)
    }
  __syncthreads();
  if (tid != 0) return;
  int m = 0;
  for (int q = 0; q < C; ++q) m += s_met[q];
  const int k = L % S;
  bool lead[kReqWords];                               // unmet and the tail is its first k tokens
  for (int q = 0; q < C; ++q) {
    lead[q] = !s_met[q];
    for (int j = 0; j < k && lead[q]; ++j) lead[q] = tok(L - k + j) == s_req[q * S + j];
  }
  base[r] = S * m;
  for (int q = 0; q < kReqWords; ++q) {
    int v = -1, dest = 0;
    if (q < C && lead[q]) {
      v = s_req[q * S + k];
      if (k + 1 < S) {
        dest = S * m + k + 1;
      } else {
        int gain = 0;
        for (int p = 0; p < C; ++p) gain += (lead[p] && s_req[p * S + k] == v) ? 1 : 0;
        dest = S * (m + gain);
      }
    }
    special[((size_t)r * kReqWords + q) * 2] = v;
    special[((size_t)r * kReqWords + q) * 2 + 1] = dest;
  }
}

// Entry b's one live slot: the first slot of bank S * (the padding rows of b), log-probability 0; every other slot
// finished with -inf.
__global__ __launch_bounds__(256) void beam_required_init_kernel(const int32_t* __restrict__ req, float* __restrict__ log_probs,
                                                                 int32_t* __restrict__ finished, int64_t* __restrict__ lengths,
                                                                 int R, int W, int C, int S) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= R) return;
  const int b = i / W, w = i - b * W, Wb = W / (C * S + 1);
  int pad = 0;
  for (int q = 0; q < C; ++q) pad += req[((size_t)b * C + q) * S] < 0 ? 1 : 0;
  const bool live = w == S * pad * Wb;
  log_probs[i] = live ? 0.f : -INFINITY;
  finished[i] = live ? 0 : 1;
  lengths[i] = 0;
}

}  // namespace

// executor-internal: what every caller of the required words checks.  cons: the constraints of the same decode, or null;
// max_steps > 0: the rules of a whole decode.
int comic_beam_required_check(const comic_beam_required* q, const char* who, int W, int V, int end_id, int max_steps,
                              const comic_beam_constraints* cons) {
  COMIC_REQUIRE(q, "%s: null required", who);
  COMIC_REQUIRE(q->n_words >= 1 && q->n_words <= kReqWords, "%s: required.n_words must be in [1,%d] (got %d)", who, kReqWords,
                q->n_words);
  COMIC_REQUIRE(q->stride >= 1 && q->stride <= kReqStride, "%s: required.stride must be in [1,%d] (got %d)", who, kReqStride,
                q->stride);
  const int banks = q->n_words * q->stride + 1;
  COMIC_REQUIRE(W >= 1 && W <= 64 && W % banks == 0, "%s: required: %d banks (n_words * stride + 1) do not divide the beam width %d",
                who, banks, W);
  COMIC_REQUIRE(V > 0 && V <= 65536, "%s: required: a vocabulary of %d words exceeds 65536", who, V);
  COMIC_REQUIRE(end_id >= 0 && end_id < V, "%s: end_id %d outside the vocabulary", who, end_id);
  if (cons && max_steps > 0)   // a live beam keeps W finite candidates: the constraints' rule, and the at most 4 specials
    COMIC_REQUIRE((long)V >= (long)W + cons->n_suppress + 1 + max_steps + kReqWords,
                  "%s: vocabulary of %d is too small for beam %d + %d suppressed + 1 + %d steps + %d required", who, V, W,
                  cons->n_suppress, max_steps, kReqWords);
  return 0;
}

// executor-internal: one launch, honouring the executor's stop flag
int comic_beam_required_launch(const int32_t* prev_words, const int32_t* prev_parents, const int32_t* req, int32_t* hist,
                               int32_t* base, int32_t* special, const comic_beam_required* q, int t, int B, int W, int V,
                               int max_steps, int write_hist, hipStream_t st) {
  const int R = B * W;
  hipLaunchKernelGGL(beam_required_kernel, dim3(R), dim3(256), 0, st, prev_words, prev_parents, req, hist, base, special,
                     q->n_words, q->stride, t, R, W, V, max_steps, write_hist, g_comic_stop.p, g_comic_stop.t);
  COMIC_LAUNCH_CHECK("beam_required");
  return 0;
}

// executor-internal: the initial state of a decode with required words
int comic_beam_required_init_launch(const int32_t* req, float* log_probs, int32_t* finished, int64_t* lengths, int B, int W,
                                    const comic_beam_required* q, hipStream_t st) {
  const int R = B * W;
  hipLaunchKernelGGL(beam_required_init_kernel, dim3((R + 255) / 256), dim3(256), 0, st, req, log_probs, finished, lengths, R, W,
                     q->n_words, q->stride);
  COMIC_LAUNCH_CHECK("beam_required init");
  return 0;
}

extern "C" int comic_beam_required_table(const int32_t* prev_words, const int32_t* prev_parents, const int32_t* req,
                                         int32_t* hist, int32_t* base, int32_t* special, const comic_beam_required* required, int t, int B, int W,
                                   int V, int max_steps, int end_id, void* stream) {
  COMIC_REQUIRE(req && hist && base && special, "beam_required: null pointer");
  COMIC_REQUIRE(B > 0 && W >= 1 && W <= 64 && (long)B * W < (1L << 31), "beam_required: bad shape");
  COMIC_REQUIRE(max_steps > 0 && t >= 0 && t < max_steps, "beam_required: step %d outside [0,%d)", t, max_steps);
  COMIC_REQUIRE(t == 0 || (prev_words && prev_parents), "beam_required: step %d needs the words and parents of step %d", t,
                t - 1);
  if (int rc = comic_beam_required_check(required, "beam_required", W, V, end_id, 0, nullptr)) return rc;
  return comic_beam_required_launch(prev_words, prev_parents, req, hist, base, special, required, t, B, W, V, max_steps, 1,
                                    (hipStream_t)stream);
}

extern "C" int comic_beam_required_init(const int32_t* req, float* log_probs, int32_t* finished, int64_t* lengths, int B, int W,
                                        int V, int end_id, const comic_beam_required* required, void* stream) {
  COMIC_REQUIRE(req && log_probs && finished && lengths, "beam_required_init: null pointer");
  COMIC_REQUIRE(B > 0 && (long)B * W < (1L << 31), "beam_required_init: bad shape");
  if (int rc = comic_beam_required_check(required, "beam_required_init", W, V, end_id, 0, nullptr)) return rc;
  return comic_beam_required_init_launch(req, log_probs, finished, lengths, B, W, required, (hipStream_t)stream);
}
