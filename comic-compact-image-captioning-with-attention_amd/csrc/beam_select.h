// Selection under the decode kernels' total order: value descending, index ascending (the lower index wins a tie, as
// tf.argmax and a stable top_k do).  Shared by decode.hip (row argmax) and beam_step.hip.
#pragma once
#include "common.h"

struct ValIdx {
  float v;
  int i;
};
constexpr int kNone = 0x7fffffff;     // the index of "no candidate": loses every tie

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

// 256-thread argmax with ONE barrier per call: wave-level butterfly, the four wave winners through LDS slots that
// alternate with `parity` (so a call needs no trailing barrier before the next one reuses the other slots).
__device__ __forceinline__ ValIdx block_argmax_1b(float v, int i, ValIdx* sh8, int parity) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (better(ov, oi, v, i)) {
      v = ov;
      i = oi;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sh8[parity * 4 + wave].v = v;
    sh8[parity * 4 + wave].i = i;
  }
  __syncthreads();
  ValIdx r = sh8[parity * 4];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const ValIdx o = sh8[parity * 4 + w];
    if (better(o.v, o.i, r.v, r.i)) r = o;
  }
  return r;
}
