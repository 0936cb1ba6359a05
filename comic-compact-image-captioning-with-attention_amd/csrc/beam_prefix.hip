// Forced-prefix decoding: the ban masks that make the beams of an image start with the tokens its caller gave, written
// before the step of rnn_decoder_beam_search (common/ops_rnn.py:49-112) ranks through them (beam_step.hip, the Bans policy).
//
// pfx [B][P] (int32, -1 padded) holds the prefix of image b; its length is the index of the first -1.  At step t row
// r = (b, w) is FORCED when t < P, 0 <= pfx[b][t] < V and the row is live (finished == 0); a table entry outside [0, V)
// is "not forced" and never an index.
//   forced ........ every bit below V set except the token's: the row may emit pfx[b][t] alone.  The mask REPLACES what
//                   the constraints put there: inside the prefix the prefix wins.  Bits at positions >= V stay zero.
//   finished ...... all zero: a finished row bans nothing
//   otherwise ..... has_bans != 0: the row keeps the mask it has (beam_bans.hip wrote it; nothing is stored);
//                   has_bans == 0: all zero (nobody wrote the block before: every word of every row is stored)
// The mask is applied after the log-softmax, so the forced token keeps the model's own step log-probability and the
// beam's total stays log p(prefix + continuation | image).
//
// One workgroup per row, as beam_bans_kernel.  A word of the mask is a function of its index alone, so nothing is
// assembled in LDS: every lane forms its words in registers and stores them, 16 bytes per lane where the row's width
// keeps its base 16-byte aligned (words % 4 == 0: 64 lanes * 16 B = one 1 KiB store instruction per wave; a row of 2048
// words is two such stores per lane), 4 bytes per lane otherwise.  No pass that zeroes global memory, no global atomics.
#include "common.h"

namespace {

constexpr int kPrefixWords = 2048;       // words of one row's mask: V <= 65 536 (beam_bans.hip's kBanWords)

// word k of a forced row's mask: all ones below V, the token's bit clear
__device__ __forceinline__ uint32_t forced_word(int k, int tok, int V) {
  const int left = V - (k << 5);                                        // bits of this word that are below V
  uint32_t m = left >= 32 ? 0xffffffffu : left <= 0 ? 0u : ((1u << left) - 1u);
  if ((tok >> 5) == k) m &= ~(1u << (tok & 31));
  return m;
}

__global__ __launch_bounds__(256) void beam_prefix_kernel(const int32_t* __restrict__ pfx, const int32_t* __restrict__ finished,
                                                          uint32_t* __restrict__ bits, int t, int W, int V, int P, int words,
                                                          int has_bans, const int32_t* __restrict__ stop, int stop_t) {
  if (comic_stopped(stop, stop_t)) return;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int b = r / W;
  const bool live = finished[r] == 0;
  const int tok = t < P ? pfx[(size_t)b * P + t] : -1;
  const bool forced = live && tok >= 0 && tok < V;
  if (!forced && live && has_bans) return;                 // the constraints' mask stands
  uint32_t* out = bits + (size_t)r * words;
  if ((words & 3) == 0) {
    uint4* out4 = reinterpret_cast<uint4*>(out);           // (r * words) % 4 == 0: 16-byte aligned with the block
    for (int q = tid; q < (words >> 2); q += 256) {
      uint4 m = make_uint4(0u, 0u, 0u, 0u);
      if (forced) {
        const int k = q << 2;
        m = make_uint4(forced_word(k, tok, V), forced_word(k + 1, tok, V), forced_word(k + 2, tok, V),
                       forced_word(k + 3, tok, V));
      }
      out4[q] = m;
    }
  } else {
    for (int k = tid; k < words; k += 256) out[k] = forced ? forced_word(k, tok, V) : 0u;
  }
}

}  // namespace

// executor-internal: one launch, honouring the executor's stop flag
int comic_beam_prefix_launch(const int32_t* pfx, const int32_t* finished, uint32_t* bits, int t, int B, int W, int V, int P,
                             int has_bans, hipStream_t st) {
  const int R = B * W, words = (V + 31) / 32;
  hipLaunchKernelGGL(beam_prefix_kernel, dim3(R), dim3(256), 0, st, pfx, finished, bits, t, W, V, P, words, has_bans ? 1 : 0,
                     g_comic_stop.p, g_comic_stop.t);
  COMIC_LAUNCH_CHECK("beam_prefix");
  return 0;
}

// executor-internal: what every caller of a prefix record checks
int comic_beam_prefix_check(const comic_beam_prefix* p, const char* who, int V, int max_steps) {
  COMIC_REQUIRE(p, "%s: null prefix", who);
  COMIC_REQUIRE(V > 0 && (V + 31) / 32 <= kPrefixWords, "%s: vocabulary of %d words needs more than %d mask words", who, V,
                kPrefixWords);
  COMIC_REQUIRE(p->max_tokens >= 1 && p->max_tokens < max_steps, "%s: max_tokens %d outside [1,%d)", who, p->max_tokens,
                max_steps);
  return 0;
}

extern "C" int comic_beam_prefix_mask(const int32_t* pfx, const int32_t* finished, uint32_t* bits, int t, int B, int W, int V,
                                      int P, int has_bans, void* stream) {
  COMIC_REQUIRE(pfx && finished && bits, "beam_prefix: null pointer");
  COMIC_REQUIRE(B > 0 && W >= 1 && W <= 64 && (long)B * W < (1L << 31), "beam_prefix: bad shape");
  COMIC_REQUIRE(V > 0 && (V + 31) / 32 <= kPrefixWords, "beam_prefix: vocabulary of %d words needs more than %d mask words", V,
                kPrefixWords);
  COMIC_REQUIRE(P >= 1, "beam_prefix: table width %d is below 1", P);
  COMIC_REQUIRE(t >= 0, "beam_prefix: step %d is negative", t);
  COMIC_REQUIRE(((uintptr_t)bits & 15) == 0, "beam_prefix: bits is not 16-byte aligned");
  return comic_beam_prefix_launch(pfx, finished, bits, t, B, W, V, P, has_bans, (hipStream_t)stream);
}
