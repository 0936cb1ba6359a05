// Soft-target cross-entropy of the teacher-forced step and the teacher's top-K table (include/comic_hip.h,
// "Soft-target XE training").
//
//   q        = (1 - eps - lam) e_y + eps / V + lam q_T        q_T(v) = sum_k [ids_k = v] probs_k / sum_k probs_k
//   loss     = wmask (lse(z) - sum_v q_v z_v)                 the cross-entropy H(q, p), not the KL divergence
//   nll      = wmask (lse(z) - z_y)                           the hard loss, for comparable perplexities
//   dlogits  = (softmax(z) - q) coef
//
// xent_soft_kernel is xent_row's passes (decoder.hip: one workgroup of 256 lanes per row, the same reductions in the same
// order, so eps = lam = 0 gives xent_row's softmax) with one more sum, of z, for the eps term, and K gathers for the
// teacher's.  teacher_topk_kernel forms the weighted mean of n members' tempered softmaxes of a row in LDS and takes its
// K largest entries by repeated arg-max, (value descending, id ascending).  No atomics, fixed summation orders.
#include "exec_entries.h"

namespace {

constexpr int kSoftMaxK = 32;                       // entries of a teacher row (COMIC_SOFT_MAX_K)
constexpr int kTopkScratch = 2 * 256 * 4;           // bytes of LDS in front of teacher_topk_kernel's row
constexpr int kTopkLdsMax = 160 * 1024;

// sum over the workgroup's 256 values in the tree order of xent_row; every lane gets the result
__device__ __forceinline__ float block_sum(float x, float* s, int tid) {
  s[tid] = x;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) s[tid] += s[tid + st];
    __syncthreads();
  }
  const float r = s[0];
  __syncthreads();
  return r;
}

// max and arg-max (ties: the lowest index) over the workgroup's 256 candidates; every lane gets the result
__device__ __forceinline__ void block_argmax(float& mx, int& mi, float* smax, int* sidx, int tid) {
  smax[tid] = mx;
  sidx[tid] = mi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      const float o = smax[tid + s];
      const int oi = sidx[tid + s];
      if (o > smax[tid] || (o == smax[tid] && oi < sidx[tid])) {
        smax[tid] = o;
        sidx[tid] = oi;
      }
    }
    __syncthreads();
  }
  mx = smax[0];
  mi = sidx[0];
  __syncthreads();
}

__global__ __launch_bounds__(256) void xent_soft_kernel(float* __restrict__ logits, const int32_t* __restrict__ targets_bt,
                                                        const float* __restrict__ coef_bt, const float* __restrict__ wmask_bt,
                                                        const int32_t* __restrict__ lens, float* __restrict__ loss_rows,
                                                        float* __restrict__ nll_rows, float* __restrict__ dlogits,
                                                        int32_t* __restrict__ ids_tb, int T, int B, int V, int ld_dl, float eps,
                                                        float lam, int K, const int32_t* __restrict__ ids_tbk,
                                                        const float* __restrict__ probs_tbk) {  // T = stride of the [B,T] tables
  __shared__ float smax[256];
  __shared__ int sidx[256];
  __shared__ float sprob[kSoftMaxK], sterm[kSoftMaxK];
  const int row = blockIdx.x, t = row / B, b = row % B, tid = threadIdx.x;
  float* lg = logits + (size_t)row * V;
  float* dl = dlogits ? dlogits + (size_t)row * ld_dl : nullptr;
  if (dl)
    for (int v = V + tid; v < ld_dl; v += 256) dl[v] = 0.f;
  if (lens && t >= lens[b]) {  // impute_finished: zero outputs
    for (int v = tid; v < V; v += 256) {
      lg[v] = 0.f;
      if (dl) dl[v] = 0.f;
    }
    if (tid == 0) {
      if (loss_rows) loss_rows[row] = 0.f;
      if (nll_rows) nll_rows[row] = 0.f;
      if (ids_tb) ids_tb[row] = 0;
    }
    return;
  }
  float mx = -INFINITY;
  int amax = 0x7fffffff;
  for (int v = tid; v < V; v += 256) {
    const float x = lg[v];
    if (x > mx) {
      mx = x;
      amax = v;
    }
  }
  block_argmax(mx, amax, smax, sidx, tid);
  float s = 0.f, sz = 0.f;
  for (int v = tid; v < V; v += 256) {
    const float x = lg[v] - mx;
    s += expf(x);
    sz += x;                                       // sum of z - max: the eps term, shifted like every other one
  }
  const float sum = block_sum(s, smax, tid);
  const float zsum = eps > 0.f ? block_sum(sz, smax, tid) : 0.f;
  // the teacher's K entries: q_T(ids_k) = probs_k / S, S summed in k order by every lane (LDS broadcasts)
  const bool teach = lam > 0.f && ids_tbk && probs_tbk;
  int my_id = -1;
  float S = 0.f, tz = 0.f;
  if (teach) {
    if (tid < K) {
      my_id = ids_tbk[(size_t)row * K + tid];
      if ((unsigned)my_id >= (unsigned)V) my_id = -1;                 // outside the contract: the entry counts for nothing
      const float pr = my_id >= 0 ? probs_tbk[(size_t)row * K + tid] : 0.f;
      sprob[tid] = pr;
      sterm[tid] = my_id >= 0 ? pr * (lg[my_id] - mx) : 0.f;
    }
    __syncthreads();
    for (int k = 0; k < K; ++k) {
      S += sprob[k];
      tz += sterm[k];
    }
  }
  const float invS = S > 0.f ? 1.f / S : 0.f;
  const int tgt = targets_bt[(size_t)b * T + t];
  const float coef = coef_bt ? coef_bt[(size_t)b * T + t] : 0.f;
  const float hard = 1.f - eps - lam, uni = eps / (float)V;
  if (dl) {
    for (int v = tid; v < V; v += 256) dl[v] = (expf(lg[v] - mx) / sum - uni - (v == tgt ? hard : 0.f)) * coef;
    if (teach) {
      __syncthreads();                             // the sweep's stores of this row, before the K read-modify-writes
      if (my_id >= 0) dl[my_id] -=lam * (sprob[tid] * invS) * coef;     // distinct ids: one lane per address
    }
  }
  if (tid == 0) {
    const float w = wmask_bt ? wmask_bt[(size_t)b * T + t] : 1.f;
    const float lse = logf(sum), zy = lg[tgt] - mx;
    if (loss_rows) loss_rows[row] = (lse - hard * zy - eps * (zsum / (float)V) - lam * (tz * invS)) * w;
    if (nll_rows) nll_rows[row] = (lse - zy) * w;
    if (ids_tb) ids_tb[row] = amax;
  }
}

struct TeacherMembers {
  const float* z[8];        // [T][B][V] logits of each member
  float w[8];
};

// One row of the table: mean probability of the members in LDS, then K arg-max picks.  Dynamic LDS:
// [256 float | 256 int | V float].
__global__ __launch_bounds__(256) void teacher_topk_kernel(TeacherMembers mem, int n, const int32_t* __restrict__ lens, int B,
                                                           int Tp, int V, float temperature, int K,
                                                           int32_t* __restrict__ ids, float* __restrict__ probs) {
  extern __shared__ __attribute__((aligned(16))) char topk_lds[];
  float* smax = (float*)topk_lds;
  int* sidx = (int*)(topk_lds + 1024);
  float* pbar = (float*)(topk_lds + kTopkScratch);
  const int row = blockIdx.x, t = row / B, b = row % B, tid = threadIdx.x;
  if (t >= Tp || t >= lens[b]) {                   // no token here: a table row the loss never reads
    if (tid < K) {
      ids[(size_t)row * K + tid] = tid;
      probs[(size_t)row * K + tid] = 0.f;
    }
    return;
  }
  for (int m = 0; m < n; ++m) {                    // members in their order; each lane owns its columns of pbar
    const float* z = mem.z[m] + (size_t)row * V;
    float mx = -INFINITY;
    int mi = 0;
    for (int v = tid; v < V; v += 256) mx = fmaxf(mx, z[v] / temperature);
    block_argmax(mx, mi, smax, sidx, tid);
    float s = 0.f;
    for (int v = tid; v < V; v += 256) s += expf(z[v] / temperature - mx);
    const float sum = block_sum(s, smax, tid);
    const float w = mem.w[m];
    for (int v = tid; v < V; v += 256) {
      const float p = w * (expf(z[v] / temperature - mx) / sum);
      pbar[v] = m == 0 ? p : pbar[v] + p;
    }
  }
  for (int k = 0; k < K; ++k) {                    // (value descending, id ascending); a taken entry becomes -1 < every p
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int v = tid; v < V; v += 256) {
      const float x = pbar[v];
      if (x > best) {
        best = x;
        bi = v;
      }
    }
    block_argmax(best, bi, smax, sidx, tid);
    if (tid == 0) {
      ids[(size_t)row * K + k] = bi;
      probs[(size_t)row * K + k] = best;
      pbar[bi] = -1.f;
    }
    __syncthreads();
  }
}

}  // namespace

int comic_xent_soft_ex(float* logits, const int32_t* targets_bt, const float* coef_bt, const float* wmask_bt,
                       const int32_t* lens, float* loss_rows, float* nll_rows, float* dlogits, int ld_dl, int32_t* ids_tb,
                       int t_rows, int t_stride, int B, int V, float smoothing, float teacher_weight, int K,
                       const int32_t* ids_tbk, const float* probs_tbk, hipStream_t st) {
  COMIC_REQUIRE(logits && targets_bt, "xent_soft: null pointer");
  COMIC_REQUIRE(B > 0 && V > 0 && t_rows > 0 && t_rows <= t_stride && ld_dl >= V, "xent_soft: bad extents");
  COMIC_REQUIRE(smoothing >= 0.f && smoothing < 1.f, "xent_soft: smoothing %g outside [0, 1)", (double)smoothing);
  COMIC_REQUIRE(teacher_weight >= 0.f && teacher_weight <= 1.f, "xent_soft: teacher_weight %g outside [0, 1]",
                (double)teacher_weight);
  COMIC_REQUIRE(smoothing + teacher_weight <= 1.f, "xent_soft: smoothing + teacher_weight = %g exceeds 1",
                (double)(smoothing + teacher_weight));
  if (teacher_weight > 0.f) {
    COMIC_REQUIRE(ids_tbk && probs_tbk, "xent_soft: teacher_weight %g without a teacher table", (double)teacher_weight);
    COMIC_REQUIRE(K >= 1 && K <= kSoftMaxK && K <= V, "xent_soft: K %d outside [1, min(%d, V)]", K, kSoftMaxK);
  }
  hipLaunchKernelGGL(xent_soft_kernel, dim3(t_rows * B), dim3(256), 0, st, logits, targets_bt, coef_bt, wmask_bt, lens,
                     loss_rows, nll_rows, dlogits, ids_tb, t_stride, B, V, ld_dl, smoothing, teacher_weight, K, ids_tbk,
                     probs_tbk);
  COMIC_LAUNCH_CHECK("xent_soft");
  return 0;
}

extern "C" int comic_xent_soft(float* logits, const int32_t* targets_bt, const float* coef_bt, const float* wmask_bt,
                               const int32_t* lens, float* loss_rows, float* nll_rows, float* dlogits, int ld_dl,
                               int32_t* ids_tb, int t_rows, int t_stride, int B, int V, float smoothing,
                               float teacher_weight, int K, const int32_t* ids_tbk, const float* probs_tbk, void* stream) {
  return comic_xent_soft_ex(logits, targets_bt, coef_bt, wmask_bt, lens, loss_rows, nll_rows, dlogits, ld_dl, ids_tb, t_rows,
                            t_stride, B, V, smoothing, teacher_weight, K, ids_tbk, probs_tbk, (hipStream_t)stream);
}

extern "C" int comic_teacher_topk(const float* const* logits, const float* weights, int n, const int32_t* lens, int B, int T,
                                  int Tp, int V, float temperature, int K, int32_t* ids, float* probs, void* stream) {
  COMIC_REQUIRE(logits && weights && lens && ids && probs, "teacher_topk: null pointer");
  COMIC_REQUIRE(n >= 1 && n <= 8, "teacher_topk: %d members outside [1, 8]", n);
  COMIC_REQUIRE(B > 0 && T > 0 && Tp > 0 && Tp <= T && V > 0, "teacher_topk: bad extents");
  COMIC_REQUIRE(K >= 1 && K <= kSoftMaxK && K <= V, "teacher_topk: K %d outside [1, min(%d, V)]", K, kSoftMaxK);
  COMIC_REQUIRE(temperature > 0.f && temperature < INFINITY, "teacher_topk: temperature %g outside (0, inf)",
                (double)temperature);
  const long lds = (long)V * 4 + kTopkScratch;
  COMIC_REQUIRE(lds <= kTopkLdsMax, "teacher_topk: a row of V = %d probabilities (%ld bytes) does not fit the %d bytes of LDS", V,
                lds, kTopkLdsMax);
  TeacherMembers mem{};
  float wsum = 0.f;
  for (int m = 0; m < n; ++m) {
    COMIC_REQUIRE(logits[m], "teacher_topk: member %d has no logits", m);
    COMIC_REQUIRE(weights[m] >= 0.f, "teacher_topk: weight %d is negative", m);
    mem.z[m] = logits[m];
    mem.w[m] = weights[m];
    wsum += weights[m];
  }
  COMIC_REQUIRE(fabsf(wsum - 1.f) <= 1e-4f, "teacher_topk: the weights sum to %g, not 1", (double)wsum);
  static PerDeviceOnce attr_once__;
  bool& attr_set = attr_once__.slot();             // hipFuncSetAttribute holds per device
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)teacher_topk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kTopkLdsMax) !=
        hipSuccess) {
      comic_set_error("teacher_topk: cannot reserve %d bytes of LDS", kTopkLdsMax);
      return 1;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL(teacher_topk_kernel, dim3(T * B), dim3(256), (size_t)lds, (hipStream_t)stream, mem, n, lens, B, Tp, V,
                     temperature, K, ids, probs);
  COMIC_LAUNCH_CHECK("teacher_topk");
  return 0;
}
