// The n-gram pieces that the consensus selection (consensus.hip) and the SCST reward (scst_reward.hip) share: the 64-bit
// key of an n-gram, the term frequency of a key among its caption's n-grams of the same order, and the idf probe.  The
// key and the table are the ones decoder.ngram_keys / decoder.NgramIdf build on the host (include/comic_hip.h,
// comic_caption_consensus: Table).  Every function is one lane's work on arrays whose element e lies at base[e * step]:
// the callers keep a caption's entries `step` apart (consensus: the candidates interleaved; the reward: contiguous).
#pragma once
#include <stdint.h>

#include "splitmix.h"

typedef unsigned long long ngram_u64;

// key of the n-gram of m tokens toks[0], toks[step], ...: h = splitmix64(m), h = splitmix64(h ^ uint64(token)); 0 -> 1
__device__ __forceinline__ ngram_u64 ngram_key(const int32_t* toks, int m, int step) {
  ngram_u64 key = splitmix64((ngram_u64)m);
  for (int s = 0; s < m; ++s) key = splitmix64(key ^ (ngram_u64)(uint32_t)toks[s * step]);
  return key ? key : 1;
}

// term frequency of the n-gram at position i among the n keys of its caption and order: the number of equal keys, or -1
// when an earlier position holds the same key (a later occurrence)
__device__ __forceinline__ double ngram_tf(const ngram_u64* keys, int n, int step, int i) {
  const ngram_u64 key = keys[i * step];
  bool later = false;
  int c = 0;
  for (int q = 0; q < n; ++q)
    if (keys[q * step] == key) {
      ++c;
      later |= q < i;
    }
  return later ? -1.0 : (double)c;
}

// g of a key: 1 without a table; with one, the stored value, or log_ref_len for a key that the table does not hold.  One
// bounded probe sequence in global memory: a table without an empty slot cannot hang it.
__device__ __forceinline__ double ngram_idf(const ngram_u64* __restrict__ tab_keys, const double* __restrict__ tab_g,
                                            long long tab_cap, double log_ref_len, ngram_u64 key) {
  if (!tab_keys) return 1.0;
  double g = log_ref_len;
  const ngram_u64 mask = (ngram_u64)tab_cap - 1;
  ngram_u64 at = key & mask;
  for (long long n = 0; n < tab_cap; ++n) {
    const ngram_u64 kk = tab_keys[at];
    if (kk == key) {
      g = tab_g[at];
      break;
    }
    if (kk == 0) break;
    at = (at + 1) & mask;
  }
  return g;
}
