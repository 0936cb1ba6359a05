// The step log-probability policies of the beam step (beam_step.hip states the rule): how a candidate's lp[v] is formed
// from the logits slab and the row constants a workgroup keeps in LDS.  One definition for every kernel that needs lp[v]:
// the beam step itself (beam_step.hip) and the truncation of the sampled step (beam_truncate.hip).
#pragma once
#include <float.h>

#include "common.h"

namespace {

struct OneMember {
  static constexpr const char* kName = "beam_step";
  static constexpr const char* kSplitName = "beam_step (split)";
  struct Rows {
    float mx[64], logsum[64];
    float lp[64];
    int fin[64];
  };
  __device__ __forceinline__ int members() const { return 1; }
  __device__ __forceinline__ void begin(Rows&) const {}
  __device__ __forceinline__ float weight(int) const { return 1.f; }
  __device__ __forceinline__ bool live(const Rows&, int) const { return true; }
  __device__ __forceinline__ float step_lp(const float* __restrict__ lg, size_t, int f, int w, const Rows& s) const {
    return (lg[f] - s.mx[w]) - s.logsum[w];
  }
};

struct Ensemble {
  static constexpr const char* kName = "beam_step_ensemble";
  static constexpr const char* kSplitName = "beam_step_ensemble (split)";
  int n;
  float w[kEnsMax];
  // Row constants of the entry: member m, beam w at [m * 64 + w]
  struct Rows {
    float mx[kEnsMax * 64], logsum[kEnsMax * 64];
    float wt[kEnsMax];
    float lp[64];
    int fin[64];
  };
  __device__ __forceinline__ int members() const { return n; }
  __device__ __forceinline__ void begin(Rows& s) const {       // the weights, visible to the workgroup on return
    if (threadIdx.x < kEnsMax) s.wt[threadIdx.x] = (int)threadIdx.x < n ? w[threadIdx.x] : 0.f;
    __syncthreads();
  }
  __device__ __forceinline__ float weight(int m) const {       // (a select chain: no dynamic index into the arguments)
    float wt = 0.f;
#pragma unroll
    for (int k = 0; k < kEnsMax; ++k)
      if (k == m) wt = w[k];
    return wt;
  }
  __device__ __forceinline__ bool live(const Rows& s, int m) const { return s.wt[m] > 0.f; }
  // member m's logits are mstride floats behind member 0's
  __device__ __forceinline__ float step_lp(const float* __restrict__ lg, size_t mstride, int f, int w, const Rows& s) const {
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
};

// host: the Ensemble policy of `n_models` members with `weights` (>= 0, finite, not all zero), checked
inline int comic_ensemble_policy(const char* who, const float* weights, int n_models, Ensemble* pol) {
  COMIC_REQUIRE(weights, "%s: null pointer", who);
  COMIC_REQUIRE(n_models >= 1 && n_models <= kEnsMax, "%s: 1 to %d members (got %d)", who, kEnsMax, n_models);
  *pol = Ensemble{};
  pol->n = n_models;
  float wsum = 0.f;
  for (int m = 0; m < n_models; ++m) {
    COMIC_REQUIRE(weights[m] >= 0.f && weights[m] <= FLT_MAX, "%s: weight %d is negative or not finite", who, m);
    pol->w[m] = weights[m];
    wsum += weights[m];
  }
  COMIC_REQUIRE(wsum > 0.f, "%s: every weight is zero", who);
  return 0;
}

}  // namespace
