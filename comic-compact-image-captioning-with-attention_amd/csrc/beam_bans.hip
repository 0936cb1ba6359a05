// Constrained beam search: the per-(entry, beam) set of banned tokens that the beam step consults (beam_step.hip, the
// Bans policy), rebuilt before every step of rnn_decoder_beam_search (common/ops_rnn.py:49-112).
//
// Row r = (b, w) of step t is the beam that step t - 1 wrote at slot w.  Its history h[0 .. t-1] is its parent's history
// plus the word step t - 1 chose for it:  H_t[b, w] = H_{t-1}[b, parent_{t-1}[b, w]] ++ word_{t-1}[b, w].  The histories
// live in beam order in two buffers hist[2][R][max_steps]; step t reads (t - 1) & 1 and writes t & 1, so a row costs
// one copy of t tokens per step and nothing walks back through the parent tree.
//
// A live row bans token v when v is suppressed, when v is <EOS> and the row is shorter than min_length, or when emitting v
// would complete an n-gram the row already holds: with L = t, (L + 1) % stride == 0 and a window start i, i % stride == 0,
// i + n - 1 <= L - 1, h[i .. i+n-2] == h[L-n+1 .. L-1], the token h[i+n-1].  A finished row bans nothing.
//
// One workgroup per row assembles the row's mask (bit v of word v / 32) in LDS and writes it out with plain stores: no
// pass that zeroes global memory, no global atomics.
#include "common.h"

namespace {

constexpr int kBanWords = 2048;          // words of one row's mask: V <= 65 536

__global__ __launch_bounds__(256) void beam_bans_kernel(const int32_t* __restrict__ prev_words,
                                                        const int32_t* __restrict__ prev_parents,
                                                        const int32_t* __restrict__ finished,
                                                        const int64_t* __restrict__ lengths, int32_t* __restrict__ hist,
                                                        uint32_t* __restrict__ bits, comic_beam_constraints c, int t, int R,
                                                        int W, int V, int max_steps, int end_id, int words,
                                                        const int32_t* __restrict__ stop, int stop_t) {
  __shared__ uint32_t s_bits[kBanWords];
  if (comic_stopped(stop, stop_t)) return;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int b = r / W;
  for (int k = tid; k < words; k += 256) s_bits[k] = 0u;
  // (a) the row's history: the parent's row of the other buffer, then the word of the step before
  const int L = t;                                  // tokens in the row's history
  const int32_t* src = nullptr;
  int last = 0;
  if (L > 0) {
    const int parent = min(max(prev_parents[r], 0), W - 1);
    last = min(max(prev_words[r], 0), V - 1);
    src = hist + ((size_t)((t - 1) & 1) * R + (size_t)b * W + parent) * max_steps;
    int32_t* dst = hist + ((size_t)(t & 1) * R + r) * max_steps;
    for (int j = tid; j < L; j += 256) dst[j] = j < L - 1 ? src[j] : last;
  }
  __syncthreads();
  const bool live = finished[r] == 0;
  if (live) {
    if (tid < c.n_suppress) {
      const int v = min(max(c.suppress[tid], 0), V - 1);
      atomicOr(&s_bits[v >> 5], 1u << (v & 31));
    }
    if (tid == 0 && lengths[r] < (int64_t)c.min_length) atomicOr(&s_bits[end_id >> 5], 1u << (end_id & 31));
    const int n = c.no_repeat_ngram, s = c.ngram_stride;
    if (n > 0 && L + 1 >= n && (L + 1) % s == 0) {
      // token j of the row: the parent's up to L - 2, the last word at L - 1 (what (a) writes; read from its sources)
      auto tok = [&](int j) { return j < L - 1 ? min(max(src[j], 0), V - 1) : last; };
      for (int i = tid * s; i + n - 1 <= L - 1; i += 256 * s) {
        bool same = true;
        for (int k = 0; k < n - 1 && same; ++k) same = tok(i + k) == tok(L - n + 1 + k);
        if (same) {
          const int v = tok(i + n - 1);
          atomicOr(&s_bits[v >> 5], 1u << (v & 31));
        }
      }
    }
  }
  __syncthreads();
  uint32_t* out = bits + (size_t)r * words;
  for (int k = tid; k < words; k += 256) out[k] = s_bits[k];
}

}  // namespace

// executor-internal: what every caller of the constraints checks.  `whole`: the rules of a whole decode (the raw operator
// builds masks for any state, so it leaves those out).
int comic_beam_constraints_check(const comic_beam_constraints* c, const char* who, int W, int V, int end_id, int max_steps,
                                 bool whole) {
  COMIC_REQUIRE(c, "%s: null constraints", who);
  COMIC_REQUIRE(V > 0 && (V + 31) / 32 <= kBanWords, "%s: vocabulary of %d words needs more than %d mask words", who, V,
                kBanWords);
  COMIC_REQUIRE(end_id >= 0 && end_id < V, "%s: end_id %d outside the vocabulary", who, end_id);
  COMIC_REQUIRE(c->min_length >= 0, "%s: min_length %d is negative", who, c->min_length);
  COMIC_REQUIRE(c->no_repeat_ngram >= 0, "%s: no_repeat_ngram %d is negative", who, c->no_repeat_ngram);
  COMIC_REQUIRE(c->ngram_stride >= 1, "%s: ngram_stride %d is below 1", who, c->ngram_stride);
  COMIC_REQUIRE(c->no_repeat_ngram % c->ngram_stride == 0, "%s: no_repeat_ngram %d is no multiple of ngram_stride %d", who,
                c->no_repeat_ngram, c->ngram_stride);
  COMIC_REQUIRE(c->n_suppress >= 0 && c->n_suppress <= 32, "%s: n_suppress %d outside [0,32]", who, c->n_suppress);
  for (int k = 0; k < c->n_suppress; ++k) {
    COMIC_REQUIRE(c->suppress[k] >= 0 && c->suppress[k] < V, "%s: suppressed id %d outside the vocabulary of %d", who,
                  c->suppress[k], V);
    COMIC_REQUIRE(c->suppress[k] != end_id, "%s: end_id %d is suppressed", who, end_id);
  }
  if (whole) {
    COMIC_REQUIRE(c->min_length < max_steps, "%s: min_length %d is not below max_steps %d", who, c->min_length, max_steps);
    // a live beam keeps W finite candidates: at most n_suppress + <EOS> + one per token of its history are banned
    COMIC_REQUIRE((long)V >= (long)W + c->n_suppress + 1 + max_steps,
                  "%s: vocabulary of %d is too small for beam %d + %d suppressed + 1 + %d steps", who, V, W, c->n_suppress,
                  max_steps);
  }
  return 0;
}

// executor-internal: one launch, honouring the executor's stop flag
int comic_beam_bans_launch(const int32_t* prev_words, const int32_t* prev_parents, const int32_t* finished,
                           const int64_t* lengths, int32_t* hist, uint32_t* bits, int t, int B, int W, int V, int max_steps,
                           int end_id, const comic_beam_constraints* c, hipStream_t st) {
  const int R = B * W, words = (V + 31) / 32;
  hipLaunchKernelGGL(beam_bans_kernel, dim3(R), dim3(256), 0, st, prev_words, prev_parents, finished, lengths, hist, bits, *c,
                     t, R, W, V, max_steps, end_id, words, g_comic_stop.p, g_comic_stop.t);
  COMIC_LAUNCH_CHECK("beam_bans");
  return 0;
}

extern "C" int comic_beam_bans(const int32_t* prev_words, const int32_t* prev_parents, const int32_t* finished,
                               const int64_t* lengths, int32_t* hist, uint32_t* bits, int t, int B, int W, int V,
                               int max_steps, int end_id, const comic_beam_constraints* constraints, void* stream) {
  COMIC_REQUIRE(finished && lengths && hist && bits, "beam_bans: null pointer");
  COMIC_REQUIRE(B > 0 && W >= 1 && W <= 64 && (long)B * W < (1L << 31), "beam_bans: bad shape");
  COMIC_REQUIRE(max_steps > 0 && t >= 0 && t < max_steps, "beam_bans: step %d outside [0,%d)", t, max_steps);
  COMIC_REQUIRE(t == 0 || (prev_words && prev_parents), "beam_bans: step %d needs the words and parents of step %d", t,
                t - 1);
  if (int rc = comic_beam_constraints_check(constraints, "beam_bans", W, V, end_id, max_steps, false)) return rc;
  return comic_beam_bans_launch(prev_words, prev_parents, finished, lengths, hist, bits, t, B, W, V, max_steps, end_id,
                                constraints, (hipStream_t)stream);
}
