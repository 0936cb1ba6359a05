// The seam between the forward (conv.hip) and the backward (conv_bwd.hip) of the CNN plan: backward-data runs the forward
// kernels, so the backward needs the forward's per-op launcher and the little both halves' kernels share.  Nothing else
// of conv.hip is visible from conv_bwd.hip.
#pragma once
#include "conv_common.h"

// the activation gradient a backward-data launch applies to its result (ConvArgs::mask_*), and where that result goes
struct ConvMask {
  const void* y;            // forward output of the producer conv, rows of y_cs channels, slice from y_co
  int y_cs, y_co;
  const float* scale;       // its BatchNorm scale
  float* dbeta;             // its d beta accumulator
  void* dz;                 // its d-conv tensor [B][Ho][Wo][Cout] (stride 1: not dilated)
};

// One op of a plan on the forward kernels (conv.hip, instantiated there for float, bf16_t and f16_t).  accum: y += result;
// mask: a plain backward-data launch whose epilogue applies the producer's activation gradient.
template <typename T>
int comic_run_op(const comic_cnn_op* op, const void* x, int xc, void* y, int yc, const comic_conv_weight* wt, int batch,
                 hipStream_t st, int accum = 0, const ConvMask* mask = nullptr);

namespace {

constexpr int kRowBytes = 80;  // 64 B of k + 16 B pad (spreads ds_read_b128 over the banks)

// one 16-byte chunk <-> Elem<T>::EPC floats
template <typename T>
__device__ __forceinline__ void load_vec(const T* p, float* v);
template <>
__device__ __forceinline__ void load_vec<float>(const float* p, float* v) {
  const float4 t = *(const float4*)p;
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
template <>
__device__ __forceinline__ void load_vec<bf16_t>(const bf16_t* p, float* v) {
  const uint4 t = *(const uint4*)p;
  const uint32_t u[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(u[i] << 16);
    v[2 * i + 1] = __uint_as_float(u[i] & 0xFFFF0000u);
  }
}
template <>
__device__ __forceinline__ void load_vec<f16_t>(const f16_t* p, float* v) {
  const uint4 t = *(const uint4*)p;
  const uint32_t u[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = Half16<f16_t>::lo(u[i]);
    v[2 * i + 1] = Half16<f16_t>::hi(u[i]);
  }
}
template <typename T>
__device__ __forceinline__ void store_vec(T* p, const float* v);
template <>
__device__ __forceinline__ void store_vec<float>(float* p, const float* v) {
  *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
}
template <>
__device__ __forceinline__ void store_vec<bf16_t>(bf16_t* p, const float* v) {
  *(uint4*)p = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                          pack_bf16x2(v[6], v[7]));
}
template <>
__device__ __forceinline__ void store_vec<f16_t>(f16_t* p, const float* v) {
  typedef Half16<f16_t> F;
  *(uint4*)p = make_uint4(F::pack(v[0], v[1]), F::pack(v[2], v[3]), F::pack(v[4], v[5]), F::pack(v[6], v[7]));
}

}  // namespace
