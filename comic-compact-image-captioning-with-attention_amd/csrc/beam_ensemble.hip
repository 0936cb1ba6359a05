// Ensemble beam step: one _beam_search_step ([TF-1.9] BeamSearchDecoder as used by common/ops_rnn.py:49-112) whose
// per-step word distribution is the weighted mean of several members' distributions.  Same state arrays and the same total
// order (value descending, flat index w * V + v ascending) as beam_step_kernel in decode.hip.
//
//   a_m[v] = (logits_m[v] - max_m) - log sum exp(logits_m - max_m)          log-softmax of member m's row
//   A      = max over the members with weight > 0 of a_m[v]
//   lp[v]  = A + log sum_m wt_m * exp(a_m[v] - A)                           members in order 0, 1, ...
//
// A member with weight 0 is never read: it contributes exactly 0 to the sum, and leaving it out of A as well keeps a
// zero-weight member with a far larger a_m from pushing every term that counts into underflow.  With one member of weight
// 1 the sum is exp(0) = 1 and lp = a_0 to the bit, the step of comic_beam_step.  Everything behind lp is that step:
// finished rows read [F32_MIN ... 0 at end_id ...], total = log_probs[w] + lp, the optional length penalty ranks by
// total / ((5 + len) / 6)^lpw while the state keeps the unpenalised total, then the finished / lengths bookkeeping.
//
// Two forms:
//   ens_step_kernel ......... one workgroup per batch entry: any V, length penalty included
//   ens_stats_kernel ........ per (chunk, beam, entry, member): max and sum exp(x - max) of the chunk
//   ens_chunk_topk_kernel ... per (entry, chunk): every member's row constants from the partials (combined in chunk order,
//                             so each workgroup of an entry gets the same bits), lp of its slice of all W beams, its top-W
//   ens_merge_kernel ........ per entry: top-W of the chunks' candidates + bookkeeping
// No kernel waits on another workgroup; the three launches of the split form are ordered by the stream.
#include <float.h>

#include <algorithm>

#include "common.h"

constexpr int kEnsMax = 8;

namespace {

struct ValIdx {
  float v;
  int i;
};
struct EnsWeights {
  float w[kEnsMax];
};
constexpr int kNone = 0x7fffffff;

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__device__ __forceinline__ ValIdx block_argmax(float v, int i, ValIdx* sh) {
  const int tid = threadIdx.x;
  sh[tid].v = v;
  sh[tid].i = i;
  __syncthreads();
  for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
    if (tid < s && better(sh[tid + s].v, sh[tid + s].i, sh[tid].v, sh[tid].i)) sh[tid] = sh[tid + s];
    __syncthreads();
  }
  const ValIdx r = sh[0];
  __syncthreads();
  return r;
}

// Row constants of the entry in LDS: member m, beam w at [m * 64 + w]
struct EnsRows {
  float mx[kEnsMax * 64], logsum[kEnsMax * 64];
  float wt[kEnsMax];
  float lp[64];
  int fin[64];
};

// lp of candidate (beam w, word v) of the entry whose member-0 logits start at lg; member m's are mstride floats further
__device__ __forceinline__ float ens_step_lp(const float* __restrict__ lg, size_t mstride, int n, int f, int w,
                                             const EnsRows& s) {
  float a[kEnsMax];
  float A = -INFINITY;
#pragma unroll
  for (int m = 0; m < kEnsMax; ++m) {
    a[m] = -INFINITY;
    if (m < n && s.wt[m] > 0.f) {
      a[m] = (lg[m * mstride + f] - s.mx[m * 64 + w]) - s.logsum[m * 64 + w];
      A = fmaxf(A, a[m]);
    }
  }
  float sum = 0.f;
#pragma unroll
  for (int m = 0; m < kEnsMax; ++m)
    if (m < n && s.wt[m] > 0.f) sum += s.wt[m] * expf(a[m] - A);      // member order 0, 1, ...
  return A + logf(sum);
}
// unpenalised total of the candidate: _mask_probs for a finished beam
__device__ __forceinline__ float ens_total(const float* __restrict__ lg, size_t mstride, int n, int f, int w, int v,
                                           int end_id, const EnsRows& s) {
  const float step = s.fin[w] ? ((v == end_id) ? 0.f : -FLT_MAX) : ens_step_lp(lg, mstride, n, f, w, s);
  return s.lp[w] + step;
}

// all-(-inf) / all-NaN corner of a selection round: the lowest untaken flat index (matches a stable sort)
__device__ __forceinline__ int lowest_untaken(const int* sel, int r) {
  int f = 0;
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

// ---- one workgroup per batch entry -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ens_step_kernel(const float* __restrict__ logits, EnsWeights wts, int n,
                                                       float* __restrict__ log_probs, int32_t* __restrict__ finished,
                                                       int64_t* __restrict__ lengths, int32_t* __restrict__ word_ids,
                                                       int32_t* __restrict__ parent_ids, float* __restrict__ scores,
                                                       int B, int W, int V, int end_id, float lpw,
                                                       const int32_t* __restrict__ stop, int stop_t) {
  __shared__ ValIdx sh[256];
  __shared__ EnsRows s;
  __shared__ int s_sel[64];
  __shared__ float s_selv[64];
  __shared__ long long s_len[64];
  if (comic_stopped(stop, stop_t)) return;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t mstride = (size_t)B * W * V;
  const float* lg = logits + (size_t)b * W * V;
  if (tid < kEnsMax) s.wt[tid] = tid < n ? wts.w[tid] : 0.f;
  for (int w = tid; w < W; w += 256) {
    s.lp[w] = log_probs[b * W + w];
    s.fin[w] = finished[b * W + w];
    s_len[w] = lengths[b * W + w];
  }
  __syncthreads();
  // log-softmax constants per (member, beam): one wave per row
  for (int p = wave; p < n * W; p += 4) {
    const int m = p / W, w = p - m * W;
    if (!(s.wt[m] > 0.f)) continue;
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
  __syncthreads();
  const int total = W * V;
  for (int r = 0; r < W; ++r) {
    float bv = -INFINITY;
    int bi = kNone;
    for (int f = tid; f < total; f += 256) {
      bool taken = false;
      for (int q = 0; q < r; ++q) taken |= (s_sel[q] == f);
      if (taken) continue;
      const int w = f / V, v = f - w * V;
      float tot = ens_total(lg, mstride, n, f, w, v, end_id, s);
      if (lpw != 0.f) {
        const long long len = s_len[w] + ((s.fin[w] || v == end_id) ? 0 : 1);
        tot = tot / powf((5.f + (float)len) / 6.f, lpw);
      }
      if (better(tot, f, bv, bi)) {
        bv = tot;
        bi = f;
      }
    }
    const ValIdx best = block_argmax(bv, bi, sh);
    if (tid == 0) {
      s_sel[r] = best.i == kNone ? lowest_untaken(s_sel, r) : best.i;
      s_selv[r] = best.v;
    }
    __syncthreads();
  }
  if (tid < W) {
    const int f = s_sel[tid];
    const int parent = f / V, word = f - parent * V;
    const int prev_fin = s.fin[parent];
    word_ids[b * W + tid] = word;
    parent_ids[b * W + tid] = parent;
    scores[b * W + tid] = s_selv[tid];
    // the state carries the unpenalised total log probability of the chosen candidate
    log_probs[b * W + tid] = lpw != 0.f ? ens_total(lg, mstride, n, f, parent, word, end_id, s) : s_selv[tid];
    finished[b * W + tid] = (prev_fin || word == end_id) ? 1 : 0;
    lengths[b * W + tid] = s_len[parent] + (prev_fin ? 0 : 1);
  }
}

// ---- large vocabularies: the step split over `chunks` workgroups per entry ------------------------------------------------
// partials at [((m * B + b) * W + w) * chunks + c]
__global__ __launch_bounds__(256) void ens_stats_kernel(const float* __restrict__ logits, EnsWeights wts,
                                                        float* __restrict__ pmax, float* __restrict__ psum, int B, int W,
                                                        int V, int chunks, const int32_t* __restrict__ stop, int stop_t) {
  if (comic_stopped(stop, stop_t)) return;
  __shared__ float sh[4];
  const int c = blockIdx.x, w = blockIdx.y, m = blockIdx.z / B, b = blockIdx.z - m * B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float wt = 0.f;
#pragma unroll
  for (int k = 0; k < kEnsMax; ++k)
    if (k == m) wt = wts.w[k];
  if (!(wt > 0.f)) return;                    // (uniform over the workgroup) a zero-weight member is never read
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

// KLOCAL > 0: a thread's share of the W * nv candidates (column v0 + tid + 256 * k of every beam) is formed ONCE, with all
// members' loads in flight together, and the W selection rounds run on the register copy; 0: the rescanning form.
template <int KLOCAL>
__global__ __launch_bounds__(256) void ens_chunk_topk_kernel(const float* __restrict__ logits, EnsWeights wts, int n,
                                                             const float* __restrict__ log_probs,
                                                             const int32_t* __restrict__ finished,
                                                             const float* __restrict__ pmax, const float* __restrict__ psum,
                                                             float* __restrict__ cand_v, int32_t* __restrict__ cand_i, int B,
                                                             int W, int V, int chunks, int end_id,
                                                             const int32_t* __restrict__ stop, int stop_t) {
  __shared__ ValIdx sh[256];
  __shared__ EnsRows s;
  __shared__ int s_sel[64];
  if (comic_stopped(stop, stop_t)) return;
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t mstride = (size_t)B * W * V;
  const float* lg = logits + (size_t)b * W * V;
  if (tid < kEnsMax) s.wt[tid] = tid < n ? wts.w[tid] : 0.f;
  for (int w = tid; w < W; w += 256) {
    s.lp[w] = log_probs[b * W + w];
    s.fin[w] = finished[b * W + w];
  }
  __syncthreads();
  // row constants from the per-chunk partials: one wave per (member, beam), one lane per chunk (chunks <= 32), partials
  // combined in chunk order so that every workgroup of the entry gets the same bits
  for (int p = wave; p < n * W; p += 4) {
    const int m = p / W, w = p - m * W;
    if (!(s.wt[m] > 0.f)) continue;
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
  __syncthreads();
  const int per = (V + chunks - 1) / chunks, v0 = c * per, v1 = min(V, v0 + per), nv = max(0, v1 - v0);
  const size_t out = ((size_t)b * chunks + c) * W;
  constexpr int kLocal = KLOCAL > 0 ? KLOCAL : 1;
  const int kper = (nv + 255) >> 8;                 // columns per thread and beam
  if (KLOCAL > 0 && W * kper <= kLocal) {
    float tv[kLocal];
    int ti[kLocal];
    int w = 0, k = 0;                               // (beam, column slot) of register slot e
#pragma unroll
    for (int e = 0; e < kLocal; ++e) {
      tv[e] = -INFINITY;
      ti[e] = kNone;
      const int v = v0 + tid + 256 * k;
      if (w < W && v < v1) {
        const int f = w * V + v;
        tv[e] = ens_total(lg, mstride, n, f, w, v, end_id, s);
        ti[e] = f;
      }
      if (++k == kper) {
        k = 0;
        ++w;
      }
    }
    for (int r = 0; r < W; ++r) {
      float bv = -INFINITY;
      int bi = kNone;
#pragma unroll
      for (int e = 0; e < kLocal; ++e)
        if (ti[e] != kNone && better(tv[e], ti[e], bv, bi)) {
          bv = tv[e];
          bi = ti[e];
        }
      const ValIdx best = block_argmax(bv, bi, sh);
#pragma unroll
      for (int e = 0; e < kLocal; ++e)
        if (ti[e] == best.i) ti[e] = kNone;         // taken (flat indices are unique; kNone marks "none")
      if (tid == 0) {
        cand_v[out + r] = best.v;
        cand_i[out + r] = best.i;
      }
    }
    return;
  }
  const int total = W * nv;
  for (int r = 0; r < W; ++r) {
    float bv = -INFINITY;
    int bi = kNone;
    for (int j = tid; j < total; j += 256) {
      const int w = j / nv, v = v0 + (j - w * nv);
      const int f = w * V + v;
      bool taken = false;
      for (int q = 0; q < r; ++q) taken |= (s_sel[q] == f);
      if (taken) continue;
      const float tot = ens_total(lg, mstride, n, f, w, v, end_id, s);
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
}

// The global top-W under a total order is the top-W of the union of the per-chunk top-W lists.
__global__ __launch_bounds__(256) void ens_merge_kernel(const float* __restrict__ cand_v, const int32_t* __restrict__ cand_i,
                                                        float* __restrict__ log_probs, int32_t* __restrict__ finished,
                                                        int64_t* __restrict__ lengths, int32_t* __restrict__ word_ids,
                                                        int32_t* __restrict__ parent_ids, float* __restrict__ scores, int W,
                                                        int V, int chunks, int end_id, const int32_t* __restrict__ stop,
                                                        int stop_t) {
  __shared__ ValIdx sh[256];
  __shared__ int s_fin[64], s_sel[64];
  __shared__ float s_selv[64];
  __shared__ long long s_len[64];
  if (comic_stopped(stop, stop_t)) return;
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int w = tid; w < W; w += 256) {
    s_fin[w] = finished[b * W + w];
    s_len[w] = lengths[b * W + w];
  }
  __syncthreads();
  const int n = chunks * W;
  const float* cv = cand_v + (size_t)b * n;
  const int32_t* ci = cand_i + (size_t)b * n;
  for (int r = 0; r < W; ++r) {
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
      s_sel[r] = best.i == kNone ? lowest_untaken(s_sel, r) : best.i;
      s_selv[r] = best.v;
    }
    __syncthreads();
  }
  if (tid < W) {
    const int f = s_sel[tid];
    const int parent = f / V, word = f - parent * V;
    const int prev_fin = s_fin[parent];
    word_ids[b * W + tid] = word;
    parent_ids[b * W + tid] = parent;
    scores[b * W + tid] = s_selv[tid];
    log_probs[b * W + tid] = s_selv[tid];
    finished[b * W + tid] = (prev_fin || word == end_id) ? 1 : 0;
    lengths[b * W + tid] = s_len[parent] + (prev_fin ? 0 : 1);
  }
}

// State re-ordering of a member that runs the per-step launch chain: out[r] = in[(r / W) * W + parent[r]] for c, h and the
// attention state in one launch.  Unlike comic_gather_rows it honours the loop's stop flag and clamps the parent: after
// the loop has ended the previous step's parents were never written.
__global__ void ens_gather_state_kernel(const float* __restrict__ c, const float* __restrict__ h, const float* __restrict__ att,
                                        const int32_t* __restrict__ parent, float* __restrict__ c_out,
                                        float* __restrict__ h_out, float* __restrict__ att_out, int R, int W, int D, int A,
                                        const int32_t* __restrict__ stop, int stop_t) {
  if (comic_stopped(stop, stop_t)) return;
  const int cols = 2 * D + A;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)R * cols) return;
  const int r = (int)(i / cols), k = (int)(i % cols);
  const int src = (r / W) * W + min(max(parent[r], 0), W - 1);
  if (k < D) c_out[(size_t)r * D + k] = c[(size_t)src * D + k];
  else if (k < 2 * D) h_out[(size_t)r * D + (k - D)] = h[(size_t)src * D + (k - D)];
  else att_out[(size_t)r * A + (k - 2 * D)] = att[(size_t)src * A + (k - 2 * D)];
}

// chunks per entry of the split form: the rule of comic_beam_step_ws
int ens_chunks(int B, int V) {
  const int chunks = std::max(1, std::min(32, 1024 / std::max(1, B)));
  return std::min(chunks, std::max(1, V / 1024));
}
int64_t ens_split_bytes(int n, int B, int W, int chunks) {
  return ((int64_t)2 * n * B * W * chunks + (int64_t)2 * B * chunks * W) * 4 + 1024;
}

thread_local int g_ens_step_path = 0;

}  // namespace

// executor-internal
int comic_ens_gather_state(const float* c, const float* h, const float* att, const int32_t* parent, float* c_out,
                           float* h_out, float* att_out, int R, int W, int D, int A, hipStream_t st) {
  const long total = (long)R * (2 * D + A);
  if (total == 0) return 0;
  hipLaunchKernelGGL(ens_gather_state_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, c, h, att, parent, c_out,
                     h_out, att_out, R, W, D, A, g_comic_stop.p, g_comic_stop.t);
  COMIC_LAUNCH_CHECK("ensemble gather_state");
  return 0;
}

extern "C" int comic_beam_step_ensemble_path(void) { return g_ens_step_path; }

extern "C" int64_t comic_beam_step_ensemble_workspace(int n_models, int B, int W, int V) {
  if (n_models < 1 || n_models > kEnsMax || B <= 0 || W <= 0 || V <= 0) return -1;
  return ens_split_bytes(n_models, B, W, ens_chunks(B, V));
}

extern "C" int comic_beam_step_ensemble(const float* logits, const float* weights, int n_models, float* log_probs,
                                        int32_t* finished, int64_t* lengths, int32_t* word_ids, int32_t* parent_ids,
                                        float* scores, int B, int W, int V, int end_id, float length_penalty_weight,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
  COMIC_REQUIRE(logits && weights && log_probs && finished && lengths && word_ids && parent_ids && scores,
                "beam_step_ensemble: null pointer");
  COMIC_REQUIRE(n_models >= 1 && n_models <= kEnsMax, "beam_step_ensemble: 1 to %d members (got %d)", kEnsMax, n_models);
  COMIC_REQUIRE(B > 0 && W >= 1 && W <= 64, "beam_step_ensemble: beam width must be in [1,64] (got %d)", W);
  COMIC_REQUIRE(V > 0 && W <= V && (long)W * V < (1L << 31), "beam_step_ensemble: beam*V too large or beam > V");
  COMIC_REQUIRE((long)n_models * B <= 65535, "beam_step_ensemble: members * batch too large");
  EnsWeights wts{};
  float wsum = 0.f;
  for (int m = 0; m < n_models; ++m) {
    COMIC_REQUIRE(weights[m] >= 0.f && weights[m] <= FLT_MAX, "beam_step_ensemble: weight %d is negative or not finite", m);
    wts.w[m] = weights[m];
    wsum += weights[m];
  }
  COMIC_REQUIRE(wsum > 0.f, "beam_step_ensemble: every weight is zero");
  hipStream_t st = (hipStream_t)stream;
  const float lpw = length_penalty_weight;
  const int chunks = ens_chunks(B, V);
  const bool split = lpw == 0.f && (long)W * V >= 8192 && chunks >= 2 && workspace &&
                     workspace_bytes >= ens_split_bytes(n_models, B, W, chunks);
  g_ens_step_path = split ? 1 : 0;
  if (!split) {
    hipLaunchKernelGGL(ens_step_kernel, dim3(B), dim3(256), 0, st, logits, wts, n_models, log_probs, finished, lengths,
                       word_ids, parent_ids, scores, B, W, V, end_id, lpw, g_comic_stop.p, g_comic_stop.t);
    COMIC_LAUNCH_CHECK("beam_step_ensemble");
    return 0;
  }
  float* pmax = (float*)workspace;
  float* psum = pmax + (size_t)n_models * B * W * chunks;
  float* cand_v = psum + (size_t)n_models * B * W * chunks;
  int32_t* cand_i = (int32_t*)(cand_v + (size_t)B * chunks * W);
  hipLaunchKernelGGL(ens_stats_kernel, dim3(chunks, W, n_models * B), dim3(256), 0, st, logits, wts, pmax, psum, B, W, V,
                     chunks, g_comic_stop.p, g_comic_stop.t);
  {
    const int per = (V + chunks - 1) / chunks, kper = (per + 255) / 256;
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(chunks, B), dim3(256), 0, st, logits, wts, n_models, (const float*)log_probs,
                         (const int32_t*)finished, (const float*)pmax, (const float*)psum, cand_v, cand_i, B, W, V, chunks,
                         end_id, g_comic_stop.p, g_comic_stop.t);
    };
    if (W * kper <= 16) launch(ens_chunk_topk_kernel<16>);
    else if (W * kper <= 40) launch(ens_chunk_topk_kernel<40>);
    else launch(ens_chunk_topk_kernel<0>);
  }
  hipLaunchKernelGGL(ens_merge_kernel, dim3(B), dim3(256), 0, st, (const float*)cand_v, (const int32_t*)cand_i, log_probs,
                     finished, lengths, word_ids, parent_ids, scores, W, V, chunks, end_id, g_comic_stop.p, g_comic_stop.t);
  COMIC_LAUNCH_CHECK("beam_step_ensemble (split)");
  return 0;
}
