// One beam-search step on a slab of logits: log-softmax, finished masking, top-k over beam * V, length / finished
// bookkeeping.  Restates [TF-1.9] _beam_search_step as used by common/ops_rnn.py:49-112:
//   log_softmax -> _mask_probs (finished rows: float32.min, 0 at EOS) -> total = log_probs[:, :, None] + step
//   -> top_k(beam) over the flattened beam * V axis -> word = idx % V, parent = idx / V.
// Candidates are ranked under one total order, value descending and flat index w * V + v ascending, within a chunk, across
// chunks and across beams.  With a length penalty (lpw != 0, _get_scores) they are ranked by
// total / ((5 + length) / 6)^lpw with length = the beam's + 1 unless the beam is finished or the candidate is EOS; the beam
// state keeps the unpenalised total, the step's `scores` output the penalised one.
//
// How a candidate's step log-probability lp[v] is formed is a policy, known at compile time:
//   OneMember ... lp[v] = (logits[v] - max) - log sum exp(logits - max)                       the row's log-softmax
//   Ensemble  ... a_m[v] = member m's log-softmax as above, A = max over the members with weight > 0 of a_m[v],
//                 lp[v] = A + log sum_m wt_m * exp(a_m[v] - A), members in order 0, 1, ...: the log of the weighted mean
//                 of the members' distributions.  A member with weight 0 is never read: it contributes exactly 0 to the
//                 sum, and leaving it out of A as well keeps a zero-weight member with a far larger a_m from pushing every
//                 term that counts into underflow.  With one member of weight 1 and finite logits the sum is exp(0) = 1
//                 and lp = a_0 to the bit.  (OneMember is NOT this with n = 1: a_0 - A is NaN at a -inf logit, a weight
//                 other than 1 adds log wt, and the single path would pay an expf / logf per candidate.)
// The policy also owns the row constants a workgroup keeps in LDS: [64] per beam for one member, [kEnsMax * 64] for several.
// (The two structs live in beam_policy.h: beam_truncate.hip forms lp[v] with the same code.)
//
// Which candidates a live beam may not emit is a second, orthogonal policy (constrained beam search):
//   NoBans ... none: the code of the step as it always was
//   Bans ..... bit v of row (b, w) of `bits` [B*W][words] (beam_bans.hip builds it before the step) bans candidate (w, v):
//              its step log-probability is -inf.  Applied AFTER the log-softmax -- the normaliser counts banned tokens,
//              so survivors keep their scores -- and to live beams only (_mask_probs is untouched).  One L2-resident word
//              load and a bit test per candidate, however many tokens are banned.
//
// How the W slots of an entry share the candidates is a third, orthogonal policy (diverse beam search, Vijayakumar et al.
// 2016, with the Hamming diversity):
//   NoGroups ... one beam of width W: the code of the step as it always was
//   Groups ..... G groups (1 <= G <= W, W % G == 0, Wg = W / G) and diversity = lambda, a finite float >= 0.  Group g owns
//                the slots [g * Wg, (g + 1) * Wg) of an entry.  total[w][v] = log_probs[w] + step[w][v] and score[w][v]
//                (total, or total / ((5 + len) / 6)^lpw) are exactly the plain step's, _mask_probs and bans included.  The
//                groups are processed in order g = 0, 1, ..., G - 1:
//                  count[v]   = the number of slots q < g * Wg of the entry whose word chosen AT THIS STEP is v
//                  rank[w][v] = score[w][v] - lambda * count[v] for a live beam w and v != end_id, else score[w][v]
//                               (a finished beam and <EOS> are never penalised: otherwise the first group to end a caption
//                               would push every later group to run on); the product float(lambda) * float(count) is
//                               formed in fp32 and subtracted once
//                  select       the group's Wg best among ITS OWN Wg * V candidates, rank descending and entry-wide flat
//                               index f = w * V + v ascending (w the entry-wide slot); in the all-(-inf) / NaN corner the
//                               lowest untaken flat index of the group's range
//                  write        slot g * Wg + r: word = f % V, parent = f / V (an entry-wide slot, always inside the
//                               group), scores = the rank, log_probs (the state) = the UNPENALISED total, finished and
//                               lengths as ever
//                Parents being entry-wide slots, gather_tree, the state gathers, the attention histories and the ban
//                histories work unchanged.  The initial state has the first slot of each group live (beam_init_kernel
//                with Wg for W).  G == 1 is the plain step; lambda == 0 is G independent beams of width Wg; group 0 is
//                always beam search of width Wg.  The penalty is per TOKEN at the same position (with radix tokens: not
//                per word).  A candidate finds its count by one bit test in an LDS mask of the penalised words (hashed by
//                v mod 32 768, so any V fits) and walks the list of at most 63 words only on a hit.
//   Samples .... W independent chains (sampling n = W captions per image): every slot of an entry is live from the start
//                (beam_init_kernel with width 1) and takes, at step t, the best of ITS OWN V candidates under
//                  rank[v] = lp[v] * inv_temp + g(b, w, t, v)      for a live slot; -inf (a ban) stays -inf
//                lowest v on ties, the lowest flat index of its row in the all-(-inf) / NaN corner.  lp[v] is the policy's
//                step_lp exactly as above, inv_temp = 1.0f / temperature formed once on the host, and g Gumbel noise from
//                a counter-based generator that nobody stores (splitmix.h; seed_dev = uint64[2] = {seed, image_base} in
//                device memory, read at run time so a captured graph replays with a new seed):
//                  k1 = splitmix64(splitmix64(seed) ^ (image_base + b))
//                  k2 = splitmix64(k1 ^ ((uint64(w) << 32) | uint64(t)))      once per (slot, step), kept in LDS
//                  r  = splitmix64(k2 ^ uint64(v)),  k = r >> 41,  u = (2k + 1) * 2^-24  (exact, never 0 or 1)
//                  g  = -logf(-logf(u))                                       the accurate logf; g in [-2.82, 16.64]
//                A finished slot sees no noise: _mask_probs makes it emit <EOS> and its log-probability carries over.
//                word = v, parent = w (the slot itself), log_probs (the state) = old state + lp[v] and scores = the same
//                value: the model's UNPERTURBED, UNTEMPERED log p(caption so far | image), which at a temperature != 1 is
//                not the log-probability under the tempered distribution.  The perturbed rank is never returned.  No
//                length penalty, no groups.  To the launches it is ONE group of all W slots whose selection round r is
//                restricted to slot r (kPerSlot): the one-workgroup form loops over the slots, the split form is the
//                statistics, one chunk launch (every slot's best per chunk, the unperturbed total beside it) and one
//                merge -- 3 launches whatever W is.  The lists hold W candidates per chunk, so the totals need a block
//                of their own in the workspace: comic_beam_step_sampled_workspace.
//
// Beam search with required words splits the W slots into banks by constraint progress.  A bank's parents are any of the W
// slots, so it is no member of the slot above (whose launches update a group's state in place) but a pair of kernels of
// its own further down ("banks by constraint progress"), built from the same step_lp, cand_step, order and write_beam.
//
// Two forms, one copy of each kernel, instantiated per policy:
//   beam_step_kernel ........ one workgroup per batch entry: any V, length penalty included
//   beam_stats_kernel ....... per (chunk, beam, entry, member): max and sum exp(x - max) of the chunk
//   beam_chunk_topk_kernel .. per (entry, chunk): every row's constants from the partials (combined in chunk order, so each
//                             workgroup of an entry gets the same bits), lp of its slice of all W beams, its own top-W
//   beam_merge_kernel ....... per entry: top-W of the chunks' candidates + bookkeeping (candidates carry totals; under
//                             Groups their ranks, and the unpenalised totals beside them)
// The global top-W under a total order is the top-W of the union of the per-chunk top-W lists.  No kernel waits on another
// workgroup; the three launches of the split form are ordered by the stream.  Under Groups the one-workgroup form loops
// over the groups inside the kernel (the words chosen so far stay in LDS); the split form runs the statistics once and
// then, per group, one chunk top-k launch over that group's beams and one merge that writes that group's slots -- 1 + 2 G
// launches, ordered by the stream -- and group g's chunk kernel reads the words of the groups before it from the step's
// own word_ids rows, where the earlier merges wrote them.  (Word tokens: V = 25 599, beam 3 -> 76 797
// candidates per entry; one workgroup per entry leaves the GPU empty and scans them 2 + W times.)
#include <float.h>

#include <algorithm>

#include "beam_policy.h"
#include "beam_select.h"
#include "splitmix.h"

// executor-internal: chunks per entry of the split form, and the bytes of its workspace for n members
// (2 * n * B * W * chunks floats of partials + B * chunks * W (float + int32) candidates)
int comic_beam_step_chunks(int B, int V) {
  const int chunks = std::max(1, std::min(32, 1024 / std::max(1, B)));
  return std::min(chunks, std::max(1, V / 1024));
}
int64_t comic_beam_step_split_bytes(int n, int B, int W, int chunks) {
  return ((int64_t)2 * n * B * W * chunks + (int64_t)2 * B * chunks * W) * 4 + 1024;
}

namespace {

struct NoBans {
  __device__ __forceinline__ NoBans entry(int, int) const { return NoBans{}; }
  __device__ __forceinline__ bool hit(int, int) const { return false; }
};
struct Bans {
  const uint32_t* bits;      // [B * W][words]
  int words;
  // the masks of entry b's W beams
  __device__ __forceinline__ Bans entry(int b, int W) const { return Bans{bits + (size_t)b * W * words, words}; }
  __device__ __forceinline__ bool hit(int w, int v) const { return (bits[(size_t)w * words + (v >> 5)] >> (v & 31)) & 1u; }
};

constexpr int kPenWords = 1024;      // LDS mask of the penalised words: bit (v mod 32 768)
struct NoGroups {
  static constexpr bool kActive = false;
  static constexpr bool kPerSlot = false;
  struct Pen {};
  __host__ __device__ __forceinline__ int groups() const { return 1; }
  __device__ __forceinline__ int group() const { return 0; }
  NoGroups at(int, float*, const int32_t*) const { return NoGroups{}; }
  __device__ __forceinline__ int chosen(int) const { return 0; }
  __device__ __forceinline__ void clear(Pen&, int, int) const {}
  __device__ __forceinline__ void add(Pen&, int, int) const {}
  __device__ __forceinline__ float rank(const Pen&, int, float score, float, bool, int, int, int) const { return score; }
  __device__ __forceinline__ void total(size_t, float) const {}
  __device__ __forceinline__ float total_of(size_t, const ValIdx& best) const { return best.v; }
};
struct Groups {
  static constexpr bool kActive = true;
  static constexpr bool kPerSlot = false;
  int G;
  float lambda;
  int g;               // split form: the group this launch serves
  float* cand_t;       // split form: the candidates' unpenalised totals, beside cand_v (their ranks)
  const int32_t* words;  // split form: the step's word_ids output, whose slots before the group are already written
  struct Pen {
    uint32_t mask[kPenWords];
    int word[64];
  };
  __host__ __device__ __forceinline__ int groups() const { return G; }
  __device__ __forceinline__ int group() const { return g; }
  // host: the policy of group g's launches of the split form
  Groups at(int group, float* totals, const int32_t* word_ids) const { return Groups{G, lambda, group, totals, word_ids}; }
  __device__ __forceinline__ int chosen(int row) const { return words[row]; }
  // (every thread; the caller's barrier makes it visible)
  __device__ __forceinline__ void clear(Pen& p, int, int) const {
    for (int k = threadIdx.x; k < kPenWords; k += blockDim.x) p.mask[k] = 0u;
  }
  // slot q of the entry chose `word` at this step
  __device__ __forceinline__ void add(Pen& p, int q, int word) const {
    p.word[q] = word;
    atomicOr(&p.mask[(word & (32 * kPenWords - 1)) >> 5], 1u << (word & 31));
  }
  // split form: the unpenalised total of candidate o of the chunk lists
  __device__ __forceinline__ void total(size_t o, float t) const { cand_t[o] = t; }
  // merge: the total of the round's winner, candidate o (none: the round's -inf)
  __device__ __forceinline__ float total_of(size_t o, const ValIdx& best) const { return best.i == kNone ? best.v : cand_t[o]; }
  // the rank of candidate v of slot w with `score` (its step log-probability `step`), npen slots before its group
  __device__ __forceinline__ float rank(const Pen& p, int npen, float score, float, bool live, int, int v, int end_id) const {
    if (!live || v == end_id || !((p.mask[(v & (32 * kPenWords - 1)) >> 5] >> (v & 31)) & 1u)) return score;
    int count = 0;
    for (int q = 0; q < npen; ++q) count += (p.word[q] == v) ? 1 : 0;
    if (count == 0) return score;
    {
#pragma clang fp contract(off)
      const float pen = lambda * (float)count;
      return score - pen;
    }
  }
};

// The generator of the Samples policy (the contract: include/comic_hip.h, comic_beam_sampling).  seed = {seed, image_base}.
__device__ __forceinline__ uint64_t sample_k2(const uint64_t* __restrict__ seed, int b, int w, int t) {
  const uint64_t k1 = splitmix64(splitmix64(seed[0]) ^ (seed[1] + (uint64_t)b));
  return splitmix64(k1 ^ (((uint64_t)w << 32) | (uint64_t)(uint32_t)t));
}
__device__ __forceinline__ int sample_k(uint64_t k2, int v) { return (int)(splitmix64(k2 ^ (uint64_t)v) >> 41); }
// u = (2k + 1) * 2^-24 is exact in fp32 and never 0 or 1; the accurate logf (the native approximation loses g near u -> 1)
__device__ __forceinline__ float sample_gumbel(int k) {
  const float u = (float)(2 * k + 1) * (1.0f / 16777216.0f);
  return -logf(-logf(u));
}
// W independent chains: every slot takes the best of ITS OWN V candidates under rank = lp * inv_temp + Gumbel noise.  One
// "group" of all W slots as far as the launches go (groups() == 1: the statistics, one chunk launch, one merge); kPerSlot
// restricts selection round r to slot r in every kernel.  The candidates carry their unperturbed totals as under Groups.
struct Samples {
  static constexpr bool kActive = true;
  static constexpr bool kPerSlot = true;
  const uint64_t* seed;  // device: {seed, image_base}, read at run time
  float inv_temp;
  int t;                 // the step
  float* cand_t;         // split form: the candidates' unperturbed totals, beside cand_v (their ranks)
  struct Pen {
    uint64_t k2[64];     // the key of (entry, slot w, step): formed once per workgroup
  };
  __host__ __device__ __forceinline__ int groups() const { return 1; }
  __device__ __forceinline__ int group() const { return 0; }
  Samples at(int, float* totals, const int32_t*) const { return Samples{seed, inv_temp, t, totals}; }
  __device__ __forceinline__ int chosen(int) const { return 0; }
  // (the caller's barrier makes it visible)
  __device__ __forceinline__ void clear(Pen& p, int b, int W) const {
    if ((int)threadIdx.x < W) p.k2[threadIdx.x] = sample_k2(seed, b, threadIdx.x, t);
  }
  __device__ __forceinline__ void add(Pen&, int, int) const {}
  __device__ __forceinline__ void total(size_t o, float tot) const { cand_t[o] = tot; }
  __device__ __forceinline__ float total_of(size_t o, const ValIdx& best) const { return best.i == kNone ? best.v : cand_t[o]; }
  // a finished slot sees no noise; -inf (a banned candidate) stays -inf
  __device__ __forceinline__ float rank(const Pen& p, int, float score, float step, bool live, int w, int v, int) const {
    if (!live) return score;
    const float g = sample_gumbel(sample_k(p.k2[w], v));
    {
#pragma clang fp contract(off)
      const float scaled = step * inv_temp;
      return scaled + g;
    }
  }
};

// step log-probability / unpenalised total of candidate (beam w, word v), flat index f, of the entry whose member-0 logits
// start at lg and whose bans are bn: _mask_probs for a finished beam, -inf for a banned candidate of a live one
template <class P, class Bn>
__device__ __forceinline__ float cand_step(const P& pol, const Bn& bn, const float* __restrict__ lg, size_t mstride, int f,
                                           int w, int v, int end_id, const typename P::Rows& s) {
  return s.fin[w] ? ((v == end_id) ? 0.f : -FLT_MAX)                                                     // dtype.min
                  : (bn.hit(w, v) ? -INFINITY : pol.step_lp(lg, mstride, f, w, s));
}
template <class P, class Bn>
__device__ __forceinline__ float cand_total(const P& pol, const Bn& bn, const float* __restrict__ lg, size_t mstride, int f,
                                            int w, int v, int end_id, const typename P::Rows& s) {
  return s.lp[w] + cand_step(pol, bn, lg, mstride, f, w, v, end_id, s);
}

// (Groups, split form) the unpenalised total of a chunk's chosen candidate f, -inf for "none"
template <class P, class Bn>
__device__ __forceinline__ float chunk_total(const P& pol, const Bn& bn, const float* __restrict__ lg, size_t mstride, int f,
                                             int V, int end_id, const typename P::Rows& s) {
  if (f == kNone) return -INFINITY;
  const int w = f / V;
  return cand_total(pol, bn, lg, mstride, f, w, f - w * V, end_id, s);
}

// all-(-inf) / all-NaN corner of a selection round: the lowest untaken flat index from `first` on (matches a stable sort)
__device__ __forceinline__ int lowest_untaken(const int* sel, int r, int first = 0) {
  int f = first;
  bool again = true;
  while (again) {
    again = false;
    for (int q = 0; q < r; ++q)
      if (sel[q] == f) {
        ++f;
        again = true;
      }
  }
  return f;
}

// the W chosen flat indices of an entry -> its outputs and new state; `total` is the unpenalised total of slot tid
__device__ __forceinline__ void write_beam(int o, int f, float score, float total, const int* fin, const long long* len, int V,
                                           int end_id, float* __restrict__ log_probs, int32_t* __restrict__ finished,
                                           int64_t* __restrict__ lengths, int32_t* __restrict__ word_ids,
                                           int32_t* __restrict__ parent_ids, float* __restrict__ scores) {
  const int parent = f / V, word = f - parent * V;
  const int prev_fin = fin[parent];
  word_ids[o] = word;
  parent_ids[o] = parent;
  scores[o] = score;
  log_probs[o] = total;
  finished[o] = (prev_fin || word == end_id) ? 1 : 0;
  lengths[o] = len[parent] + (prev_fin ? 0 : 1);
}

// The row constants of an entry's W beams (every member), into the workgroup's LDS rows; the caller's barrier makes them
// visible.  From the logits: one wave per (member, beam) row, max and log sum exp(x - max) over the V logits.
template <class P>
__device__ __forceinline__ void rows_from_logits(const P& pol, typename P::Rows& s, const float* __restrict__ lg, size_t mstride,
                                                 int W, int V) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int p = wave; p < pol.members() * W; p += 4) {
    const int m = pol.members() > 1 ? p / W : 0, w = p - m * W;
    if (!pol.live(s, m)) continue;
    const float* row = lg + m * mstride + (size_t)w * V;
    float mx = -INFINITY;
    for (int v = lane; v < V; v += 64) mx = fmaxf(mx, row[v]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int v = lane; v < V; v += 64) sum += expf(row[v] - mx);
    sum = wave_sum(sum);
    if (lane == 0) {
      s.mx[m * 64 + w] = mx;
      s.logsum[m * 64 + w] = logf(sum);
    }
  }
}
// From the per-chunk partials of beam_stats_kernel: one wave per (member, beam), one lane per chunk (chunks <= 32), partials
// combined in chunk order so that every workgroup of the entry gets the same bits
template <class P>
__device__ __forceinline__ void rows_from_partials(const P& pol, typename P::Rows& s, const float* __restrict__ pmax,
                                                   const float* __restrict__ psum, int B, int b, int W, int chunks) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int p = wave; p < pol.members() * W; p += 4) {
    const int m = pol.members() > 1 ? p / W : 0, w = p - m * W;
    if (!pol.live(s, m)) continue;
    const size_t o = (((size_t)m * B + b) * W + w) * chunks;
    const float pm = lane < chunks ? pmax[o + lane] : -INFINITY;
    const float ps = lane < chunks ? psum[o + lane] : 0.f;
    const float mx = wave_max(pm);
    const float term = lane < chunks ? ps * expf(pm - mx) : 0.f;
    float sum = 0.f;
    for (int k = 0; k < chunks; ++k) sum += __shfl(term, k, 64);      // fixed order: chunk 0, 1, ...
    if (lane == 0) {
      s.mx[m * 64 + w] = mx;
      s.logsum[m * 64 + w] = logf(sum);
    }
  }
}

// ---- one workgroup per batch entry -----------------------------------------------------------------------------------
template <class P, class Bn, class Gr>
__global__ __launch_bounds__(256) void beam_step_kernel(const float* __restrict__ logits, P pol, Bn bans, float* __restrict__ log_probs,
                                                        int32_t* __restrict__ finished, int64_t* __restrict__ lengths,
                                                        int32_t* __restrict__ word_ids, int32_t* __restrict__ parent_ids,
                                                        float* __restrict__ scores, int B, int W, int V, int end_id,
                                                        float lpw, const int32_t* __restrict__ stop, int stop_t, Gr gr) {
  __shared__ ValIdx sh[256];
  __shared__ typename P::Rows s;
  __shared__ int s_sel[64];
  __shared__ float s_selv[64];
  __shared__ long long s_len[64];
  __shared__ typename Gr::Pen pen;
  if (comic_stopped(stop, stop_t)) return;
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t mstride = (size_t)B * W * V;
  const float* lg = logits + (size_t)b * W * V;
  const Bn bn = bans.entry(b, W);
  gr.clear(pen, b, W);
  // the entry's beam state (W <= 64): loaded first, in flight behind the passes over the logits
  float lp_w = 0.f;
  int fin_w = 0;
  long long len_w = 0;
  if (tid < W) {
    lp_w = log_probs[b * W + tid];
    fin_w = finished[b * W + tid];
    len_w = lengths[b * W + tid];
  }
  pol.begin(s);
  rows_from_logits(pol, s, lg, mstride, W, V);
  if (tid < W) {
    s.lp[tid] = lp_w;
    s.fin[tid] = fin_w;
    s_len[tid] = len_w;
  }
  __syncthreads();
  // group g selects its Wg slots among the candidates of its own Wg beams (NoGroups: one group, the W beams; Samples: one
  // group whose round r is slot r's best among its own V candidates)
  const int Wg = Gr::kActive ? W / gr.groups() : W, total = Wg * V;
  int g = 0;
  do {
    const int w0 = Gr::kActive ? g * Wg : 0, f0 = w0 * V;
    if (Gr::kActive && g > 0) {                     // the words of the group before: penalised from here on
      if (tid >= w0 - Wg && tid < w0) gr.add(pen, tid, s_sel[tid] % V);
      __syncthreads();
    }
    for (int r = 0; r < Wg; ++r) {
      float bv = -INFINITY;
      int bi = kNone;
      const int fa = Gr::kPerSlot ? r * V : f0, fb = Gr::kPerSlot ? fa + V : f0 + total;
      for (int f = fa + tid; f < fb; f += 256) {
        bool taken = false;
        for (int q = 0; q < (Gr::kPerSlot ? 0 : r); ++q) taken |= (s_sel[w0 + q] == f);
        if (taken) continue;
        const int w = f / V, v = f - w * V;
        const float step = cand_step(pol, bn, lg, mstride, f, w, v, end_id, s);
        float tot = s.lp[w] + step;
        if (lpw != 0.f) {
          const long long len = s_len[w] + ((s.fin[w] || v == end_id) ? 0 : 1);
          tot = tot / powf((5.f + (float)len) / 6.f, lpw);
        }
        if (Gr::kActive) tot = gr.rank(pen, w0, tot, step, !s.fin[w], w, v, end_id);
        if (better(tot, f, bv, bi)) {
          bv = tot;
          bi = f;
        }
      }
      const ValIdx best = block_argmax(bv, bi, sh);
      if (tid == 0) {
        s_sel[w0 + r] = best.i != kNone ? best.i : Gr::kPerSlot ? r * V : lowest_untaken(s_sel + w0, r, f0);
        s_selv[w0 + r] = best.v;
      }
      __syncthreads();
    }
  } while (Gr::kActive && ++g < gr.groups());
  if (tid < W) {
    const int f = s_sel[tid], parent = f / V, word = f - parent * V;
    // the state carries the unpenalised total log probability of the chosen candidate
    const float state = (Gr::kActive || lpw != 0.f) ? cand_total(pol, bn, lg, mstride, f, parent, word, end_id, s) : s_selv[tid];
    // (Samples: the perturbed rank is never returned; scores is the state)
    write_beam(b * W + tid, f, Gr::kPerSlot ? state : s_selv[tid], state, s.fin, s_len, V, end_id, log_probs, finished, lengths,
               word_ids, parent_ids, scores);
  }
}

// ---- large vocabularies: the step split over `chunks` workgroups per entry ------------------------------------------------
// partials at [((m * B + b) * W + w) * chunks + c]
template <class P>
__global__ __launch_bounds__(256) void beam_stats_kernel(const float* __restrict__ logits, P pol, float* __restrict__ pmax,
                                                         float* __restrict__ psum, int B, int W, int V, int chunks,
                                                         const int32_t* __restrict__ stop, int stop_t) {
  if (comic_stopped(stop, stop_t)) return;
  __shared__ float sh[4];
  const int c = blockIdx.x, w = blockIdx.y, m = pol.members() > 1 ? blockIdx.z / B : 0, b = blockIdx.z - m * B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (!(pol.weight(m) > 0.f)) return;         // (uniform over the workgroup) a zero-weight member is never read
  const int per = (V + chunks - 1) / chunks, v0 = c * per, v1 = min(V, v0 + per);
  const size_t rowi = ((size_t)m * B + b) * W + w;
  const float* row = logits + rowi * V;
  float mx = -INFINITY;
  for (int v = v0 + tid; v < v1; v += 256) mx = fmaxf(mx, row[v]);
  mx = wave_max(mx);
  if (lane == 0) sh[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  __syncthreads();
  float sum = 0.f;
  for (int v = v0 + tid; v < v1; v += 256) sum += expf(row[v] - mx);
  sum = wave_sum(sum);
  if (lane == 0) sh[wave] = sum;
  __syncthreads();
  if (tid == 0) {
    pmax[rowi * chunks + c] = mx;
    psum[rowi * chunks + c] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  }
}

// KLOCAL > 0: a thread's share of the W * nv candidates (column v0 + tid + 256 * k of every beam) fits in KLOCAL registers.
// It is formed ONCE, with all loads in flight together, and the W selection rounds run on the register copy (the
// rescanning form pays an L2 round trip per element and round: 31 -> 9 us at W = 3, V = 25 599).  0: the rescanning form.
// The launcher picks the capacity (16 / 40 / 0).  Under Groups a launch serves group gr.group(): its Wg beams, its top-Wg,
// the words of the slots before the group read from the step's word_ids (the earlier groups' merges wrote them).  The
// group policy is the LAST argument of every kernel: the others keep their places.
template <class P, class Bn, class Gr, int KLOCAL>
__global__ __launch_bounds__(256) void beam_chunk_topk_kernel(const float* __restrict__ logits, P pol, Bn bans,
                                                              const float* __restrict__ log_probs,
                                                              const int32_t* __restrict__ finished,
                                                              const float* __restrict__ pmax, const float* __restrict__ psum,
                                                              float* __restrict__ cand_v, int32_t* __restrict__ cand_i, int B,
                                                              int W, int V, int chunks, int end_id,
                                                              const int32_t* __restrict__ stop, int stop_t, Gr gr) {
  __shared__ ValIdx sh[256];
  __shared__ typename P::Rows s;
  __shared__ int s_sel[64];
  __shared__ typename Gr::Pen pen;
  if (comic_stopped(stop, stop_t)) return;
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const size_t mstride = (size_t)B * W * V;
  const float* lg = logits + (size_t)b * W * V;
  const Bn bn = bans.entry(b, W);
  const int Wg = W / gr.groups(), w0 = gr.group() * Wg;       // this launch's beams: [w0, w0 + Wg)
  if (Gr::kActive) {
    gr.clear(pen, b, W);
    __syncthreads();
    if (tid < w0) gr.add(pen, tid, gr.chosen(b * W + tid));   // (visible behind the barrier below)
  }
  // the entry's beam state (W <= 64): loaded first, in flight behind the partials
  float lp_w = 0.f;
  int fin_w = 0;
  if (tid < W) {
    lp_w = log_probs[b * W + tid];
    fin_w = finished[b * W + tid];
  }
  pol.begin(s);
  rows_from_partials(pol, s, pmax, psum, B, b, W, chunks);
  if (tid < W) {
    s.lp[tid] = lp_w;
    s.fin[tid] = fin_w;
  }
  __syncthreads();
  const int per = (V + chunks - 1) / chunks, v0 = c * per, v1 = min(V, v0 + per), nv = max(0, v1 - v0);
  const size_t out = ((size_t)b * chunks + c) * Wg;
  constexpr int kLocal = KLOCAL > 0 ? KLOCAL : 1;
  const int kper = (nv + 255) >> 8;                 // columns per thread and beam
  if (KLOCAL > 0 && Wg * kper <= kLocal) {
    __shared__ ValIdx sh8[8];
    float tv[kLocal];
    int ti[kLocal];
    int w = w0, k = 0;                              // (beam, column slot) of register slot e: scalar counters
#pragma unroll
    for (int e = 0; e < kLocal; ++e) {
      tv[e] = -INFINITY;
      ti[e] = kNone;
      const int v = v0 + tid + 256 * k;
      if (w < w0 + Wg && v < v1) {
        const int f = w * V + v;
        const float step = cand_step(pol, bn, lg, mstride, f, w, v, end_id, s);
        tv[e] = gr.rank(pen, w0, s.lp[w] + step, step, !s.fin[w], w, v, end_id);
        ti[e] = f;
      }
      if (++k == kper) {
        k = 0;
        ++w;
      }
    }
    int mine = kNone;                               // (Groups) thread r keeps round r's winner
    for (int r = 0; r < Wg; ++r) {
      float bv = -INFINITY;
      int bi = kNone;
      int ws = 0, ks = 0;                           // (Samples) the slot of register slot e: round r takes slot r's best
#pragma unroll
      for (int e = 0; e < kLocal; ++e) {
        if ((!Gr::kPerSlot || ws == r) && ti[e] != kNone && better(tv[e], ti[e], bv, bi)) {
          bv = tv[e];
          bi = ti[e];
        }
        if (Gr::kPerSlot && ++ks == kper) {
          ks = 0;
          ++ws;
        }
      }
      const ValIdx best = block_argmax_1b(bv, bi, sh8, r & 1);
      if (!Gr::kPerSlot) {
#pragma unroll
        for (int e = 0; e < kLocal; ++e)
          if (ti[e] == best.i) ti[e] = kNone;       // taken (flat indices are unique; kNone marks "none")
      }
      if (tid == 0) {
        cand_v[out + r] = best.v;
        cand_i[out + r] = best.i;
      }
      if (Gr::kActive && tid == r) mine = best.i;
    }
    if (Gr::kActive && tid < Wg) gr.total(out + tid, chunk_total(pol, bn, lg, mstride, mine, V, end_id, s));
    return;
  }
  const int total = Gr::kPerSlot ? nv : Wg * nv;    // (Samples: round r scans slot r's columns)
  for (int r = 0; r < Wg; ++r) {
    float bv = -INFINITY;
    int bi = kNone;
    for (int j = tid; j < total; j += 256) {
      const int wl = Gr::kPerSlot ? r : j / nv, w = w0 + wl, v = v0 + (Gr::kPerSlot ? j : j - wl * nv);
      const int f = w * V + v;
      bool taken = false;
      for (int q = 0; q < (Gr::kPerSlot ? 0 : r); ++q) taken |= (s_sel[q] == f);
      if (taken) continue;
      const float step = cand_step(pol, bn, lg, mstride, f, w, v, end_id, s);
      const float tot = gr.rank(pen, w0, s.lp[w] + step, step, !s.fin[w], w, v, end_id);
      if (better(tot, f, bv, bi)) {
        bv = tot;
        bi = f;
      }
    }
    const ValIdx best = block_argmax(bv, bi, sh);
    if (tid == 0) {
      s_sel[r] = best.i;                            // kNone when the chunk has fewer than r + 1 candidates
      cand_v[out + r] = best.v;
      cand_i[out + r] = best.i;
    }
    __syncthreads();
  }
  if (Gr::kActive && tid < Wg) gr.total(out + tid, chunk_total(pol, bn, lg, mstride, s_sel[tid], V, end_id, s));
}

// Under Groups a launch merges group gr.group()'s lists (Wg per chunk, ranked) into that group's slots; the state takes
// the chosen candidate's unpenalised total from gr.cand_t.
template <class Gr>
__global__ __launch_bounds__(256) void beam_merge_kernel(const float* __restrict__ cand_v, const int32_t* __restrict__ cand_i,
                                                         float* __restrict__ log_probs, int32_t* __restrict__ finished,
                                                         int64_t* __restrict__ lengths, int32_t* __restrict__ word_ids,
                                                         int32_t* __restrict__ parent_ids, float* __restrict__ scores, int W,
                                                         int V, int chunks, int end_id, const int32_t* __restrict__ stop,
                                                         int stop_t, Gr gr) {
  __shared__ ValIdx sh[256];
  __shared__ int s_fin[64], s_sel[64];
  __shared__ float s_selv[64];
  __shared__ float s_selt[Gr::kActive ? 64 : 1];
  __shared__ long long s_len[64];
  if (comic_stopped(stop, stop_t)) return;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < W) {                       // (W <= 64)
    s_fin[tid] = finished[b * W + tid];
    s_len[tid] = lengths[b * W + tid];
  }
  __syncthreads();
  const int Wg = W / gr.groups(), w0 = gr.group() * Wg;
  const int n = chunks * Wg;
  const float* cv = cand_v + (size_t)b * n;
  const int32_t* ci = cand_i + (size_t)b * n;
  if (Gr::kPerSlot) {                  // slot tid's best over the chunks' lists (one candidate per chunk and slot)
    if (tid < W) {
      float bv = -INFINITY;
      int bi = kNone, bj = 0;
      for (int c = 0; c < chunks; ++c) {
        const int j = c * W + tid, f = ci[j];
        if (f != kNone && better(cv[j], f, bv, bi)) {
          bv = cv[j];
          bi = f;
          bj = j;
        }
      }
      const float tot = gr.total_of((size_t)b * n + bj, ValIdx{bv, bi});
      write_beam(b * W + tid, bi == kNone ? tid * V : bi, tot, tot, s_fin, s_len, V, end_id, log_probs, finished, lengths,
                 word_ids, parent_ids, scores);
    }
    return;
  }
  for (int r = 0; r < Wg; ++r) {
    float bv = -INFINITY;
    int bi = kNone, bj = 0;
    for (int j = tid; j < n; j += 256) {
      const int f = ci[j];
      if (f == kNone) continue;
      bool taken = false;
      for (int q = 0; q < r; ++q) taken |= (s_sel[q] == f);
      if (taken) continue;
      if (better(cv[j], f, bv, bi)) {
        bv = cv[j];
        bi = f;
        bj = j;
      }
    }
    const ValIdx best = block_argmax(bv, bi, sh);
    if (tid == 0) {
      s_sel[r] = best.i == kNone ? lowest_untaken(s_sel, r, w0 * V) : best.i;
      s_selv[r] = best.v;
    }
    // (flat indices are unique: one thread holds the winner)
    if (Gr::kActive && (best.i == kNone ? tid == 0 : bi == best.i)) s_selt[r] = gr.total_of((size_t)b * n + bj, best);
    __syncthreads();
  }
  if (tid < Wg)
    write_beam(b * W + w0 + tid, s_sel[tid], s_selv[tid], Gr::kActive ? s_selt[tid] : s_selv[tid], s_fin, s_len, V, end_id,
               log_probs, finished, lengths, word_ids, parent_ids, scores);
}

// ---- banks by constraint progress (required words; the rule: include/comic_hip.h, comic_beam_required) ---------------------
// The W slots of an entry are `banks` banks of Wb = W / banks.  A candidate (w, v) has a destination bank: a finished
// parent's own bank w / Wb; a live parent's base[w], or the dest of the first of its at most four specials that names v
// (the per-step table of beam_required.hip).  Bank c takes its Wb best among the candidates of ALL W parents whose
// destination is c and whose total is finite, under the order of every other step (score descending, flat index ascending),
// and a slot for which none is left becomes a dead slot.  step_lp, cand_step, the order and write_beam are those of the
// other steps, so a candidate's score has the same bits here.  Two forms, as the other policies:
//   beam_step_banks_kernel .. one workgroup per entry: any V, length penalty included
//   split ................... beam_stats_kernel once, then per bank beam_bank_chunk_kernel (per (chunk, entry): the rows
//                             whose base is the bank in full minus their specials, of every other live row only the specials
//                             that lead into the bank) and beam_bank_merge_kernel: 1 + 2 banks launches ordered by the
//                             stream.  A bank's parents are any of the W slots, so no launch may see the state a bank
//                             before it wrote: bank 0's chunk launch copies the entry's state into the workspace, and every
//                             later launch of the step reads that copy.
constexpr int kSpecials = 4;
struct BankRows {          // the entry's rows of the per-step table: 2 KB of specials + the bases
  int base[64];
  int tok[64 * kSpecials], dst[64 * kSpecials];
};
// (every thread; the caller's barrier makes it visible)  A token outside [0, V) is an unused special.
__device__ __forceinline__ void bank_rows_load(BankRows& t, const int32_t* __restrict__ base, const int32_t* __restrict__ special,
                                               int b, int W, int V) {
  for (int i = threadIdx.x; i < W * kSpecials; i += blockDim.x) {
    const size_t o = ((size_t)b * W * kSpecials + i) * 2;
    const int tok = special[o];
    t.tok[i] = (tok >= 0 && tok < V) ? tok : -1;
    t.dst[i] = special[o + 1];
  }
  if ((int)threadIdx.x < W) t.base[threadIdx.x] = base[b * W + threadIdx.x];
}
// the destination of candidate v of the LIVE row w
__device__ __forceinline__ int bank_dest(const BankRows& t, int w, int v) {
  int d = t.base[w];
#pragma unroll
  for (int k = kSpecials - 1; k >= 0; --k)
    if (t.tok[w * kSpecials + k] == v) d = t.dst[w * kSpecials + k];       // (the first special that names v decides)
  return d;
}
// special k of row w is in use and the first of its row to name its token
__device__ __forceinline__ bool bank_special_first(const BankRows& t, int w, int k) {
  const int tok = t.tok[w * kSpecials + k];
  bool first = tok >= 0;
  for (int q = 0; q < k; ++q) first = first && t.tok[w * kSpecials + q] != tok;
  return first;
}
// row w is scanned in full for bank c (Wb slots per bank)
__device__ __forceinline__ bool bank_full_row(const BankRows& t, const int* fin, int w, int Wb, int c) {
  return fin[w] ? (w / Wb == c) : (t.base[w] == c);
}
// a slot no eligible candidate is left for
__device__ __forceinline__ void write_dead(int o, int slot, long long len, int end_id, float* __restrict__ log_probs,
                                           int32_t* __restrict__ finished, int64_t* __restrict__ lengths,
                                           int32_t* __restrict__ word_ids, int32_t* __restrict__ parent_ids,
                                           float* __restrict__ scores) {
  word_ids[o] = end_id;
  parent_ids[o] = slot;
  scores[o] = -INFINITY;
  log_probs[o] = -INFINITY;
  finished[o] = 1;
  lengths[o] = len;
}

template <class P, class Bn>
__global__ __launch_bounds__(256) void beam_step_banks_kernel(const float* __restrict__ logits, P pol, Bn bans, float* __restrict__ log_probs,
                                                              int32_t* __restrict__ finished, int64_t* __restrict__ lengths,
                                                              int32_t* __restrict__ word_ids, int32_t* __restrict__ parent_ids,
                                                              float* __restrict__ scores, const int32_t* __restrict__ base,
                                                              const int32_t* __restrict__ special, int B, int W, int V, int end_id,
                                                              float lpw, int banks, const int32_t* __restrict__ stop, int stop_t) {
  __shared__ ValIdx sh[256];
  __shared__ typename P::Rows s;
  __shared__ BankRows tb;
  __shared__ int s_sel[64];
  __shared__ float s_selv[64];
  __shared__ long long s_len[64];
  if (comic_stopped(stop, stop_t)) return;
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t mstride = (size_t)B * W * V;
  const float* lg = logits + (size_t)b * W * V;
  const Bn bn = bans.entry(b, W);
  float lp_w = 0.f;
  int fin_w = 0;
  long long len_w = 0;
  if (tid < W) {
    lp_w = log_probs[b * W + tid];
    fin_w = finished[b * W + tid];
    len_w = lengths[b * W + tid];
  }
  pol.begin(s);
  rows_from_logits(pol, s, lg, mstride, W, V);
  bank_rows_load(tb, base, special, b, W, V);
  if (tid < W) {
    s.lp[tid] = lp_w;
    s.fin[tid] = fin_w;
    s_len[tid] = len_w;
  }
  __syncthreads();
  const int Wb = W / banks;
  for (int c = 0; c < banks; ++c) {
    const int* taken_sel = s_sel + c * Wb;
    for (int r = 0; r < Wb; ++r) {
      float bv = -INFINITY;
      int bi = kNone;
      auto consider = [&](int w, int v) {
        const int f = w * V + v;
        bool taken = false;
        for (int q = 0; q < r; ++q) taken |= (taken_sel[q] == f);
        if (taken) return;
        float tot = s.lp[w] + cand_step(pol, bn, lg, mstride, f, w, v, end_id, s);
        if (!(tot > -INFINITY)) return;                 // -inf or NaN: not eligible
        if (lpw != 0.f) {
          const long long len = s_len[w] + ((s.fin[w] || v == end_id) ? 0 : 1);
          tot = tot / powf((5.f + (float)len) / 6.f, lpw);
        }
        if (better(tot, f, bv, bi)) {
          bv = tot;
          bi = f;
        }
      };
      for (int w = 0; w < W; ++w) {
        const bool fin = s.fin[w] != 0;
        if (bank_full_row(tb, s.fin, w, Wb, c)) {
          for (int v = tid; v < V; v += 256)
            if (fin || bank_dest(tb, w, v) == c) consider(w, v);
        } else if (!fin && tid < kSpecials) {
          if (tb.dst[w * kSpecials + tid] == c && bank_special_first(tb, w, tid)) consider(w, tb.tok[w * kSpecials + tid]);
        }
      }
      const ValIdx best = block_argmax(bv, bi, sh);
      if (tid == 0) {
        s_sel[c * Wb + r] = best.i;                     // kNone: a dead slot
        s_selv[c * Wb + r] = best.v;
      }
      __syncthreads();
    }
  }
  if (tid < W) {
    const int f = s_sel[tid];
    if (f == kNone) {
      write_dead(b * W + tid, tid, s_len[tid], end_id, log_probs, finished, lengths, word_ids, parent_ids, scores);
    } else {
      const int parent = f / V, word = f - parent * V;
      const float state = lpw != 0.f ? cand_total(pol, bn, lg, mstride, f, parent, word, end_id, s) : s_selv[tid];
      write_beam(b * W + tid, f, s_selv[tid], state, s.fin, s_len, V, end_id, log_probs, finished, lengths, word_ids, parent_ids,
                 scores);
    }
  }
}

// Bank c's chunk launch (no length penalty: the score is the total).  A thread's share of the full rows' columns
// (nfull * kper values) is formed once in registers when it fits in KLOCAL, as beam_chunk_topk_kernel does; else every
// round rescans.  The at most 4 W specials of the other live rows are one candidate per thread.
template <class P, class Bn, int KLOCAL>
__global__ __launch_bounds__(256) void beam_bank_chunk_kernel(const float* __restrict__ logits, P pol, Bn bans,
                                                              const float* __restrict__ src_lp, const int32_t* __restrict__ src_fin,
                                                              const int64_t* __restrict__ src_len, float* __restrict__ snap_lp,
                                                              int32_t* __restrict__ snap_fin, int64_t* __restrict__ snap_len,
                                                              const int32_t* __restrict__ base, const int32_t* __restrict__ special,
                                                              const float* __restrict__ pmax, const float* __restrict__ psum,
                                                              float* __restrict__ cand_v, int32_t* __restrict__ cand_i, int B,
                                                              int W, int V, int chunks, int end_id, int banks, int c,
                                                              const int32_t* __restrict__ stop, int stop_t) {
  __shared__ ValIdx sh[256];
  __shared__ ValIdx sh8[8];
  __shared__ typename P::Rows s;
  __shared__ BankRows tb;
  __shared__ int s_sel[64];
  __shared__ int s_full[64];
  __shared__ int s_nfull;
  if (comic_stopped(stop, stop_t)) return;
  const int ch = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const size_t mstride = (size_t)B * W * V;
  const float* lg = logits + (size_t)b * W * V;
  const Bn bn = bans.entry(b, W);
  float lp_w = 0.f;
  int fin_w = 0;
  if (tid < W) {
    lp_w = src_lp[b * W + tid];
    fin_w = src_fin[b * W + tid];
    if (snap_lp && ch == 0) {                           // bank 0: the state every later launch of the step reads
      snap_lp[b * W + tid] = lp_w;
      snap_fin[b * W + tid] = fin_w;
      snap_len[b * W + tid] = src_len[b * W + tid];
    }
  }
  pol.begin(s);
  rows_from_partials(pol, s, pmax, psum, B, b, W, chunks);
  bank_rows_load(tb, base, special, b, W, V);
  if (tid < W) {
    s.lp[tid] = lp_w;
    s.fin[tid] = fin_w;
  }
  __syncthreads();
  const int Wb = W / banks;
  if (tid == 0) {
    int n = 0;
    for (int w = 0; w < W; ++w)
      if (bank_full_row(tb, s.fin, w, Wb, c)) s_full[n++] = w;
    s_nfull = n;
  }
  __syncthreads();
  const int nfull = s_nfull;
  const int per = (V + chunks - 1) / chunks, v0 = ch * per, v1 = min(V, v0 + per), nv = max(0, v1 - v0);
  const size_t out = ((size_t)b * chunks + ch) * Wb;
  // total of candidate (w, v), kNone when it is not eligible for the bank
  auto eligible = [&](int w, int v, float& tot) {
    if (!s.fin[w] && bank_dest(tb, w, v) != c) return kNone;
    const int f = w * V + v;
    tot = cand_total(pol, bn, lg, mstride, f, w, v, end_id, s);
    return tot > -INFINITY ? f : kNone;                 // -inf or NaN: not eligible
  };
  // the special this thread owns: special tid % 4 of row tid / 4, when its row is not scanned in full
  float sv = -INFINITY;
  int si = kNone;
  if (tid < W * kSpecials) {
    const int w = tid / kSpecials, k = tid - w * kSpecials;
    if (!s.fin[w] && tb.base[w] != c && tb.dst[tid] == c && bank_special_first(tb, w, k)) {
      const int v = tb.tok[tid];
      if (v >= v0 && v < v1) si = eligible(w, v, sv);
      if (si == kNone) sv = -INFINITY;
    }
  }
  const int kper = (nv + 255) >> 8;                     // columns per thread and row
  if (nfull * kper <= KLOCAL) {
    float tv[KLOCAL];
    int ti[KLOCAL];
    int li = 0, k = 0;
#pragma unroll
    for (int e = 0; e < KLOCAL; ++e) {
      tv[e] = -INFINITY;
      ti[e] = kNone;
      const int v = v0 + tid + 256 * k;
      if (li < nfull && v < v1) {
        ti[e] = eligible(s_full[li], v, tv[e]);
        if (ti[e] == kNone) tv[e] = -INFINITY;
      }
      if (++k == kper) {
        k = 0;
        ++li;
      }
    }
    for (int r = 0; r < Wb; ++r) {
      float bv = si != kNone ? sv : -INFINITY;
      int bi = si;
#pragma unroll
      for (int e = 0; e < KLOCAL; ++e)
        if (ti[e] != kNone && better(tv[e], ti[e], bv, bi)) {
          bv = tv[e];
          bi = ti[e];
        }
      const ValIdx best = block_argmax_1b(bv, bi, sh8, r & 1);
#pragma unroll
      for (int e = 0; e < KLOCAL; ++e)
        if (ti[e] == best.i) ti[e] = kNone;             // taken (flat indices are unique; kNone marks "none")
      if (si == best.i) si = kNone;
      if (tid == 0) {
        cand_v[out + r] = best.v;
        cand_i[out + r] = best.i;
      }
    }
    return;
  }
  const int total = nfull * nv;
  for (int r = 0; r < Wb; ++r) {
    float bv = -INFINITY;
    int bi = kNone;
    if (si != kNone) {
      bool taken = false;
      for (int q = 0; q < r; ++q) taken |= (s_sel[q] == si);
      if (!taken) {
        bv = sv;
        bi = si;
      }
    }
    for (int j = tid; j < total; j += 256) {
      const int li = j / nv, w = s_full[li], v = v0 + (j - li * nv);
      const int f = w * V + v;
      bool taken = false;
      for (int q = 0; q < r; ++q) taken |= (s_sel[q] == f);
      if (taken) continue;
      float tot;
      if (eligible(w, v, tot) != kNone && better(tot, f, bv, bi)) {
        bv = tot;
        bi = f;
      }
    }
    const ValIdx best = block_argmax(bv, bi, sh);
    if (tid == 0) {
      s_sel[r] = best.i;                                // kNone when the chunk has fewer than r + 1 candidates
      cand_v[out + r] = best.v;
      cand_i[out + r] = best.i;
    }
    __syncthreads();
  }
}

// Bank c's merge: the Wb best of the chunks' lists into the bank's slots, on the state copy of the step's first launch.
__global__ __launch_bounds__(256) void beam_bank_merge_kernel(const float* __restrict__ cand_v, const int32_t* __restrict__ cand_i,
                                                              const int32_t* __restrict__ snap_fin,
                                                              const int64_t* __restrict__ snap_len, float* __restrict__ log_probs,
                                                              int32_t* __restrict__ finished, int64_t* __restrict__ lengths,
                                                              int32_t* __restrict__ word_ids, int32_t* __restrict__ parent_ids,
                                                              float* __restrict__ scores, int W, int V, int chunks, int end_id,
                                                              int banks, int c, const int32_t* __restrict__ stop, int stop_t) {
  __shared__ ValIdx sh[256];
  __shared__ int s_fin[64], s_sel[64];
  __shared__ float s_selv[64];
  __shared__ long long s_len[64];
  if (comic_stopped(stop, stop_t)) return;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < W) {                       // (W <= 64)
    s_fin[tid] = snap_fin[b * W + tid];
    s_len[tid] = snap_len[b * W + tid];
  }
  __syncthreads();
  const int Wb = W / banks, n = chunks * Wb;
  const float* cv = cand_v + (size_t)b * n;
  const int32_t* ci = cand_i + (size_t)b * n;
  for (int r = 0; r < Wb; ++r) {
    float bv = -INFINITY;
    int bi = kNone;
    for (int j = tid; j < n; j += 256) {
      const int f = ci[j];
      if (f == kNone) continue;
      bool taken = false;
      for (int q = 0; q < r; ++q) taken |= (s_sel[q] == f);
      if (taken) continue;
      if (better(cv[j], f, bv, bi)) {
        bv = cv[j];
        bi = f;
      }
    }
    const ValIdx best = block_argmax(bv, bi, sh);
    if (tid == 0) {
      s_sel[r] = best.i;                                // kNone: a dead slot
      s_selv[r] = best.v;
    }
    __syncthreads();
  }
  if (tid < Wb) {
    const int slot = c * Wb + tid, o = b * W + slot;
    if (s_sel[tid] == kNone)
      write_dead(o, slot, s_len[slot], end_id, log_probs, finished, lengths, word_ids, parent_ids, scores);
    else
      write_beam(o, s_sel[tid], s_selv[tid], s_selv[tid], s_fin, s_len, V, end_id, log_probs, finished, lengths, word_ids,
                 parent_ids, scores);
  }
}

thread_local int g_ens_step_path = 0;

// The ONE launcher: one workgroup per entry, or -- without a length penalty (it ranks by score, not by log probability),
// with enough candidates, at least two chunks and a workspace that holds the partials -- the split form.  Under Groups
// the split form is the statistics once, then a chunk top-k and a merge per group; the eligibility rule is the same, on
// the entry-wide W * V, and the register-resident chunk form is chosen on Wg * kper.
template <class P, class Bn, class Gr>
int beam_step_launch(const P& pol, const Bn& bans, Gr gr, int n, const float* logits, float* log_probs, int32_t* finished, int64_t* lengths,
                     int32_t* word_ids, int32_t* parent_ids, float* scores, int B, int W, int V, int end_id, float lpw, void* ws,
                     int64_t ws_bytes, hipStream_t st, int* path) {
  const int chunks = comic_beam_step_chunks(B, V);
  const bool split = lpw == 0.f && (long)W * V >= 8192 && chunks >= 2 && ws &&
                     ws_bytes >= comic_beam_step_split_bytes(n, B, W, chunks) + (Gr::kPerSlot ? (int64_t)B * chunks * W * 4 : 0);
  if (path) *path = split ? 1 : 0;
  if (!split) {
    hipLaunchKernelGGL((beam_step_kernel<P, Bn, Gr>), dim3(B), dim3(256), 0, st, logits, pol, bans, log_probs, finished, lengths, word_ids,
                       parent_ids, scores, B, W, V, end_id, lpw, g_comic_stop.p, g_comic_stop.t, gr);
    COMIC_LAUNCH_CHECK(P::kName);
    return 0;
  }
  float* pmax = (float*)ws;
  float* psum = pmax + (size_t)n * B * W * chunks;
  float* cand_v = psum + (size_t)n * B * W * chunks;
  // (Samples: W candidates per chunk, so their totals take a block of their own between the ranks and the indices)
  int32_t* cand_i = (int32_t*)(cand_v + (size_t)B * chunks * W * (Gr::kPerSlot ? 2 : 1));
  hipLaunchKernelGGL(beam_stats_kernel<P>, dim3(chunks, W, n * B), dim3(256), 0, st, logits, pol, pmax, psum, B, W, V, chunks,
                     g_comic_stop.p, g_comic_stop.t);
  // (Groups: the lists are Wg <= W / 2 per chunk, so the totals fit behind the ranks inside cand_v's W per chunk)
  const int Wg = W / gr.groups();
  for (int g = 0; g < gr.groups(); ++g) {
    const Gr gg = gr.at(g, cand_v + (size_t)B * chunks * Wg, word_ids);
    const int per = (V + chunks - 1) / chunks, kper = (per + 255) / 256;
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(chunks, B), dim3(256), 0, st, logits, pol, bans, (const float*)log_probs,
                         (const int32_t*)finished, (const float*)pmax, (const float*)psum, cand_v, cand_i, B, W, V, chunks,
                         end_id, g_comic_stop.p, g_comic_stop.t, gg);
    };
    if (Wg * kper <= 16) launch(beam_chunk_topk_kernel<P, Bn, Gr, 16>);
    else if (Wg * kper <= 40) launch(beam_chunk_topk_kernel<P, Bn, Gr, 40>);
    else launch(beam_chunk_topk_kernel<P, Bn, Gr, 0>);
    hipLaunchKernelGGL(beam_merge_kernel<Gr>, dim3(B), dim3(256), 0, st, (const float*)cand_v, (const int32_t*)cand_i,
                       log_probs, finished, lengths, word_ids, parent_ids, scores, W, V, chunks, end_id, g_comic_stop.p,
                       g_comic_stop.t, gg);
  }
  COMIC_LAUNCH_CHECK(P::kSplitName);
  return 0;
}

}  // namespace

// executor-internal: the single-member step with BeamSearchDecoder's length penalty (length_penalty_weight; 0 = none) and
// a workspace (may be null) for the split form
int comic_beam_step_ws(const float* logits, float* log_probs, int32_t* finished, int64_t* lengths, int32_t* word_ids,
                       int32_t* parent_ids, float* scores, int B, int W, int V, int end_id, float lpw, void* ws,
                       int64_t ws_bytes, hipStream_t st) {
  COMIC_REQUIRE(logits && log_probs && finished && lengths && word_ids && parent_ids && scores,
                "beam_step: null pointer");
  COMIC_REQUIRE(W >= 1 && W <= 64, "beam_step: beam width must be in [1,64] (got %d)", W);
  COMIC_REQUIRE((long)W * V < (1L << 31) && W <= V, "beam_step: beam*V too large or beam > V");
  return beam_step_launch(OneMember{}, NoBans{}, NoGroups{}, 1, logits, log_probs, finished, lengths, word_ids, parent_ids, scores, B, W, V, end_id,
                          lpw, ws, ws_bytes, st, nullptr);
}
extern "C" int comic_beam_step(const float* logits, float* log_probs, int32_t* finished, int64_t* lengths,
                               int32_t* word_ids, int32_t* parent_ids, float* scores, int B, int W, int V, int end_id,
                               void* stream) {
  return comic_beam_step_ws(logits, log_probs, finished, lengths, word_ids, parent_ids, scores, B, W, V, end_id, 0.f, nullptr,
                            0, (hipStream_t)stream);
}

extern "C" int comic_beam_step_ensemble_path(void) { return g_ens_step_path; }

extern "C" int64_t comic_beam_step_ensemble_workspace(int n_models, int B, int W, int V) {
  if (n_models < 1 || n_models > kEnsMax || B <= 0 || W <= 0 || V <= 0) return -1;
  return comic_beam_step_split_bytes(n_models, B, W, comic_beam_step_chunks(B, V));
}

// the ensemble step's argument checks and launch; bits null: no bans (the code of comic_beam_step_ensemble as it was);
// grp null or one group: no groups (G == 1 IS the plain step: the same instantiation, the same launches); smp: the Samples
// policy of a sampled step (then grp is null and the penalty weight 0)
static int ens_step(const char* who, const float* logits, const float* weights, int n_models, float* log_probs,
                    int32_t* finished, int64_t* lengths, int32_t* word_ids, int32_t* parent_ids, float* scores, int B, int W,
                    int V, int end_id, float length_penalty_weight, const uint32_t* bits, int words,
                    const comic_beam_groups* grp, void* workspace, int64_t workspace_bytes, void* stream,
                    const Samples* smp = nullptr) {
  COMIC_REQUIRE(logits && weights && log_probs && finished && lengths && word_ids && parent_ids && scores,
                "%s: null pointer", who);
  COMIC_REQUIRE(n_models >= 1 && n_models <= kEnsMax, "%s: 1 to %d members (got %d)", who, kEnsMax, n_models);
  COMIC_REQUIRE(B > 0 && W >= 1 && W <= 64, "%s: beam width must be in [1,64] (got %d)", who, W);
  COMIC_REQUIRE(V > 0 && W <= V && (long)W * V < (1L << 31), "%s: beam*V too large or beam > V", who);
  COMIC_REQUIRE((long)n_models * B <= 65535, "%s: members * batch too large", who);
  Ensemble pol{};
  if (int rc = comic_ensemble_policy(who, weights, n_models, &pol)) return rc;
  if (smp) {
    if (bits)
      return beam_step_launch(pol, Bans{bits, words}, *smp, n_models, logits, log_probs, finished, lengths, word_ids, parent_ids,
                              scores, B, W, V, end_id, 0.f, workspace, workspace_bytes, (hipStream_t)stream, &g_ens_step_path);
    return beam_step_launch(pol, NoBans{}, *smp, n_models, logits, log_probs, finished, lengths, word_ids, parent_ids, scores, B,
                            W, V, end_id, 0.f, workspace, workspace_bytes, (hipStream_t)stream, &g_ens_step_path);
  }
  if (grp && grp->groups > 1) {
    const Groups gr{grp->groups, grp->diversity, 0, nullptr, nullptr};
    if (bits)
      return beam_step_launch(pol, Bans{bits, words}, gr, n_models, logits, log_probs, finished, lengths, word_ids, parent_ids,
                              scores, B, W, V, end_id, length_penalty_weight, workspace, workspace_bytes, (hipStream_t)stream,
                              &g_ens_step_path);
    return beam_step_launch(pol, NoBans{}, gr, n_models, logits, log_probs, finished, lengths, word_ids, parent_ids, scores, B,
                            W, V, end_id, length_penalty_weight, workspace, workspace_bytes, (hipStream_t)stream,
                            &g_ens_step_path);
  }
  if (bits)
    return beam_step_launch(pol, Bans{bits, words}, NoGroups{}, n_models, logits, log_probs, finished, lengths, word_ids, parent_ids, scores,
                            B, W, V, end_id, length_penalty_weight, workspace, workspace_bytes, (hipStream_t)stream,
                            &g_ens_step_path);
  return beam_step_launch(pol, NoBans{}, NoGroups{}, n_models, logits, log_probs, finished, lengths, word_ids, parent_ids, scores, B, W, V,
                          end_id, length_penalty_weight, workspace, workspace_bytes, (hipStream_t)stream, &g_ens_step_path);
}

extern "C" int comic_beam_step_ensemble(const float* logits, const float* weights, int n_models, float* log_probs,
                                        int32_t* finished, int64_t* lengths, int32_t* word_ids, int32_t* parent_ids,
                                        float* scores, int B, int W, int V, int end_id, float length_penalty_weight,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
  return ens_step("beam_step_ensemble", logits, weights, n_models, log_probs, finished, lengths, word_ids, parent_ids, scores,
                  B, W, V, end_id, length_penalty_weight, nullptr, 0, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int comic_beam_step_constrained(const float* logits, const float* weights, int n_models, float* log_probs,
                                           int32_t* finished, int64_t* lengths, int32_t* word_ids, int32_t* parent_ids,
                                           float* scores, int B, int W, int V, int end_id, float length_penalty_weight,
                                           const uint32_t* bits, int words, void* workspace, int64_t workspace_bytes,
                                           void* stream) {
  COMIC_REQUIRE(bits, "beam_step_constrained: null ban mask");
  COMIC_REQUIRE(V > 0 && words == (V + 31) / 32, "beam_step_constrained: %d mask words for a vocabulary of %d", words, V);
  return ens_step("beam_step_constrained", logits, weights, n_models, log_probs, finished, lengths, word_ids, parent_ids,
                  scores, B, W, V, end_id, length_penalty_weight, bits, words, nullptr, workspace, workspace_bytes, stream);
}

// executor-internal (decoder_exec.hip checks a loop's groups once, in front of its first launch)
int comic_beam_groups_check(const comic_beam_groups* g, const char* who, int W, int V) {
  COMIC_REQUIRE(g, "%s: null groups", who);
  COMIC_REQUIRE(g->groups >= 1, "%s: groups must be at least 1 (got %d)", who, g->groups);
  COMIC_REQUIRE(g->groups <= W, "%s: groups %d exceeds the beam width %d", who, g->groups, W);
  COMIC_REQUIRE(W % g->groups == 0, "%s: groups %d does not divide the beam width %d", who, g->groups, W);
  COMIC_REQUIRE(g->diversity >= 0.f && g->diversity <= FLT_MAX, "%s: diversity is negative or not finite", who);
  COMIC_REQUIRE(W / g->groups <= V, "%s: groups: a group's width %d exceeds V = %d", who, W / g->groups, V);
  return 0;
}

extern "C" int comic_beam_step_diverse(const float* logits, const float* weights, int n_models, float* log_probs,
                                       int32_t* finished, int64_t* lengths, int32_t* word_ids, int32_t* parent_ids,
                                       float* scores, int B, int W, int V, int end_id, float length_penalty_weight,
                                       const uint32_t* bits, int words, const comic_beam_groups* groups, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  COMIC_REQUIRE(W >= 1 && W <= 64 && V > 0, "beam_step_diverse: beam width must be in [1,64] (got %d)", W);
  if (int rc = comic_beam_groups_check(groups, "beam_step_diverse", W, V)) return rc;
  COMIC_REQUIRE(!bits || words == (V + 31) / 32, "beam_step_diverse: %d mask words for a vocabulary of %d", words, V);
  return ens_step("beam_step_diverse", logits, weights, n_models, log_probs, finished, lengths, word_ids, parent_ids, scores,
                  B, W, V, end_id, length_penalty_weight, bits, words, groups, workspace, workspace_bytes, stream);
}

// ---- sampling inside the step ------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void beam_sample_noise_kernel(const uint64_t* __restrict__ seed, int W, int t, int V, long n,
                                                                int32_t* __restrict__ k_out, float* __restrict__ g_out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int row = (int)(i / V), v = (int)(i - (long)row * V), b = row / W, w = row - b * W;
  const int k = sample_k(sample_k2(seed, b, w, t), v);
  if (k_out) k_out[i] = k;
  if (g_out) g_out[i] = sample_gumbel(k);
}
}  // namespace

// executor-internal (decoder_exec.hip checks a loop's sampling once, in front of its first launch)
int comic_beam_sampling_check(const comic_beam_sampling* s, const char* who, float lpw, int W) {
  COMIC_REQUIRE(s, "%s: null sampling", who);
  COMIC_REQUIRE(s->seed_dev, "%s: null seed_dev", who);
  COMIC_REQUIRE(s->temperature > 0.f && s->temperature <= FLT_MAX, "%s: temperature must be finite and > 0", who);
  COMIC_REQUIRE(1.0f / s->temperature <= FLT_MAX, "%s: the reciprocal of the temperature is not finite", who);
  COMIC_REQUIRE(lpw == 0.f, "%s: a length penalty does not combine with sampling", who);
  COMIC_REQUIRE(W >= 1 && W <= 64, "%s: the number of samples must be in [1,64] (got %d)", who, W);
  return 0;
}

extern "C" int comic_beam_sample_noise(const uint64_t* seed_dev, int B, int W, int t, int V, int32_t* k_out, float* g_out,
                                       void* stream) {
  COMIC_REQUIRE(seed_dev, "beam_sample_noise: null seed_dev");
  COMIC_REQUIRE(k_out || g_out, "beam_sample_noise: no output");
  COMIC_REQUIRE(B > 0 && W >= 1 && W <= 64 && V > 0 && t >= 0, "beam_sample_noise: bad shape");
  const long n = (long)B * W * V;
  COMIC_REQUIRE(n < (1L << 31), "beam_sample_noise: B*W*V too large");
  hipLaunchKernelGGL(beam_sample_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed_dev, W,
                     t, V, n, k_out, g_out);
  COMIC_LAUNCH_CHECK("beam_sample_noise");
  return 0;
}

extern "C" int64_t comic_beam_step_sampled_workspace(int n_models, int B, int W, int V) {
  if (n_models < 1 || n_models > kEnsMax || B <= 0 || W <= 0 || V <= 0) return -1;
  const int chunks = comic_beam_step_chunks(B, V);
  return comic_beam_step_split_bytes(n_models, B, W, chunks) + (int64_t)B * chunks * W * 4;
}

extern "C" int comic_beam_step_sampled(const float* logits, const float* weights, int n_models, float* log_probs,
                                       int32_t* finished, int64_t* lengths, int32_t* word_ids, int32_t* parent_ids,
                                       float* scores, int B, int W, int V, int end_id, const uint32_t* bits, int words,
                                       const comic_beam_sampling* sampling, int t, void* workspace, int64_t workspace_bytes,
                                       void* stream) {
  if (int rc = comic_beam_sampling_check(sampling, "beam_step_sampled", 0.f, W)) return rc;
  COMIC_REQUIRE(t >= 0, "beam_step_sampled: negative step %d", t);
  COMIC_REQUIRE(!bits || (V > 0 && words == (V + 31) / 32), "beam_step_sampled: %d mask words for a vocabulary of %d", words, V);
  const Samples smp{sampling->seed_dev, 1.0f / sampling->temperature, t, nullptr};
  return ens_step("beam_step_sampled", logits, weights, n_models, log_probs, finished, lengths, word_ids, parent_ids, scores,
                  B, W, V, end_id, 0.f, bits, words, nullptr, workspace, workspace_bytes, stream, &smp);
}

// ---- banks by constraint progress: the launcher and the raw operator ---------------------------------------------------------
// executor-internal: the bytes of the banked step's workspace -- the split form's, then the state copy [B * W] of
// (int64 length, float log-probability, int32 finished)
int64_t comic_beam_step_required_bytes(int n, int B, int W, int chunks) {
  return ((comic_beam_step_split_bytes(n, B, W, chunks) + 15) & ~(int64_t)15) + (int64_t)B * W * 16;
}

namespace {
template <class P, class Bn>
int beam_step_banks_launch(const P& pol, const Bn& bans, int n, const float* logits, float* log_probs, int32_t* finished,
                           int64_t* lengths, int32_t* word_ids, int32_t* parent_ids, float* scores, const int32_t* base,
                           const int32_t* special, int banks, int B, int W, int V, int end_id, float lpw, void* ws,
                           int64_t ws_bytes, hipStream_t st, int* path) {
  const int chunks = comic_beam_step_chunks(B, V);
  const bool split = lpw == 0.f && (long)W * V >= 8192 && chunks >= 2 && ws &&
                     ws_bytes >= comic_beam_step_required_bytes(n, B, W, chunks);
  if (path) *path = split ? 1 : 0;
  if (!split) {
    hipLaunchKernelGGL((beam_step_banks_kernel<P, Bn>), dim3(B), dim3(256), 0, st, logits, pol, bans, log_probs, finished, lengths,
                       word_ids, parent_ids, scores, base, special, B, W, V, end_id, lpw, banks, g_comic_stop.p, g_comic_stop.t);
    COMIC_LAUNCH_CHECK("beam_step_required");
    return 0;
  }
  float* pmax = (float*)ws;
  float* psum = pmax + (size_t)n * B * W * chunks;
  float* cand_v = psum + (size_t)n * B * W * chunks;
  int32_t* cand_i = (int32_t*)(cand_v + (size_t)B * chunks * W);
  char* snap = (char*)ws + ((comic_beam_step_split_bytes(n, B, W, chunks) + 15) & ~(int64_t)15);
  int64_t* snap_len = (int64_t*)snap;
  float* snap_lp = (float*)(snap_len + (size_t)B * W);
  int32_t* snap_fin = (int32_t*)(snap_lp + (size_t)B * W);
  hipLaunchKernelGGL(beam_stats_kernel<P>, dim3(chunks, W, n * B), dim3(256), 0, st, logits, pol, pmax, psum, B, W, V, chunks,
                     g_comic_stop.p, g_comic_stop.t);
  const int per = (V + chunks - 1) / chunks, kper = (per + 255) / 256;
  for (int c = 0; c < banks; ++c) {
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(chunks, B), dim3(256), 0, st, logits, pol, bans,
                         c == 0 ? (const float*)log_probs : (const float*)snap_lp,
                         c == 0 ? (const int32_t*)finished : (const int32_t*)snap_fin,
                         c == 0 ? (const int64_t*)lengths : (const int64_t*)snap_len, c == 0 ? snap_lp : (float*)nullptr,
                         c == 0 ? snap_fin : (int32_t*)nullptr, c == 0 ? snap_len : (int64_t*)nullptr, base, special,
                         (const float*)pmax, (const float*)psum, cand_v, cand_i, B, W, V, chunks, end_id, banks, c,
                         g_comic_stop.p, g_comic_stop.t);
    };
    // (the capacity by the most rows a bank can scan in full, W; a bank with more than fit rescans)
    if (W * kper <= 16) launch(beam_bank_chunk_kernel<P, Bn, 16>);
    else launch(beam_bank_chunk_kernel<P, Bn, 40>);
    hipLaunchKernelGGL(beam_bank_merge_kernel, dim3(B), dim3(256), 0, st, (const float*)cand_v, (const int32_t*)cand_i,
                       (const int32_t*)snap_fin, (const int64_t*)snap_len, log_probs, finished, lengths, word_ids, parent_ids,
                       scores, W, V, chunks, end_id, banks, c, g_comic_stop.p, g_comic_stop.t);
  }
  COMIC_LAUNCH_CHECK("beam_step_required (split)");
  return 0;
}
}  // namespace

extern "C" int64_t comic_beam_step_required_workspace(int n_models, int B, int W, int V) {
  if (n_models < 1 || n_models > kEnsMax || B <= 0 || W <= 0 || V <= 0) return -1;
  return comic_beam_step_required_bytes(n_models, B, W, comic_beam_step_chunks(B, V));
}

extern "C" int comic_beam_step_required(const float* logits, const float* weights, int n_models, float* log_probs,
                                        int32_t* finished, int64_t* lengths, int32_t* word_ids, int32_t* parent_ids,
                                        float* scores, int B, int W, int V, int end_id, float length_penalty_weight,
                                        const uint32_t* bits, int words, const int32_t* base, const int32_t* special, int banks,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "beam_step_required";
  COMIC_REQUIRE(logits && weights && log_probs && finished && lengths && word_ids && parent_ids && scores && base && special,
                "%s: null pointer", who);
  COMIC_REQUIRE(n_models >= 1 && n_models <= kEnsMax, "%s: 1 to %d members (got %d)", who, kEnsMax, n_models);
  COMIC_REQUIRE(B > 0 && W >= 1 && W <= 64, "%s: beam width must be in [1,64] (got %d)", who, W);
  COMIC_REQUIRE(V > 0 && W <= V && (long)W * V < (1L << 31), "%s: beam*V too large or beam > V", who);
  COMIC_REQUIRE((long)n_models * B <= 65535, "%s: members * batch too large", who);
  COMIC_REQUIRE(end_id >= 0 && end_id < V, "%s: end_id %d outside the vocabulary", who, end_id);
  COMIC_REQUIRE(banks >= 2 && banks <= 17, "%s: banks must be in [2,17] (got %d)", who, banks);
  COMIC_REQUIRE(W % banks == 0, "%s: banks %d does not divide the beam width %d", who, banks, W);
  COMIC_REQUIRE(!bits || words == (V + 31) / 32, "%s: %d mask words for a vocabulary of %d", who, words, V);
  Ensemble pol{};
  if (int rc = comic_ensemble_policy(who, weights, n_models, &pol)) return rc;
  if (bits)
    return beam_step_banks_launch(pol, Bans{bits, words}, n_models, logits, log_probs, finished, lengths, word_ids, parent_ids,
                                  scores, base, special, banks, B, W, V, end_id, length_penalty_weight, workspace,
                                  workspace_bytes, (hipStream_t)stream, &g_ens_step_path);
  return beam_step_banks_launch(pol, NoBans{}, n_models, logits, log_probs, finished, lengths, word_ids, parent_ids, scores, base,
                                special, banks, B, W, V, end_id, length_penalty_weight, workspace, workspace_bytes,
                                (hipStream_t)stream, &g_ens_step_path);
}
