// CNN encoder kernels for gfx950: implicit-GEMM convolution on MFMA with a folded
// BatchNorm + ReLU epilogue, the Cin=3 stem convolution, and the pooling kernels.
//
// Replaces the TF-1.9 op call-sites of slim.conv2d / slim.max_pool2d / slim.avg_pool2d in
// common/nets/inception_v3.py:100-415 under inception_arg_scope
// (common/nets/inception_utils.py:32-82): Conv2D (no bias) -> FusedBatchNorm(inference,
// no gamma, eps 1e-3) -> Relu, NHWC.
//
// Implicit GEMM, "swapped" orientation so that the accumulator holds 4 consecutive output
// channels of one pixel per lane (one 8-byte bf16 store):
//     D[n][m] = sum_k  Wp[n][k] * im2col(X)[m][k]        n = cout, m = (b,ho,wo), k = (kh,kw,cin)
// MFMA A-operand rows = weights, B-operand columns = pixels.  Both operands are staged in
// LDS as [row][64 bytes of k] (+16 B row padding); a lane's fragment is one 16-byte chunk
// (row = lane&15, chunk = lane>>4): 8 bf16 for v_mfma_f32_16x16x32_bf16, or 4 floats fed to
// four v_mfma_f32_16x16x4_f32 (exact fp32 parity mode; both operands use the same
// k-permutation so the sum over k is unchanged).
//
// This file is the forward of the plan; the backward (cnn_finetune) is conv_bwd.hip, and conv_run.h is all the two share.
#include "conv_run.h"
#include "conv_ws.h"
#include "conv_stem.h"
#include "conv_img.h"
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <vector>

namespace {

template <typename T, int BM, int BN, int WM, int WN, bool MASK = false>
__global__ __launch_bounds__(256) void conv_igemm_kernel(ConvArgs a) {
  constexpr int EPC = Elem<T>::EPC;
  constexpr int BKE = 4 * EPC;  // k elements per tile (64 bytes per row)
  constexpr int A_PASSES = (BM + 63) / 64;
  constexpr int B_PASSES = (BN + 63) / 64;
  constexpr int TM = BM / WM / 16;
  constexpr int TN = BN / WN / 16;
  static_assert(WM * WN == 4, "4 waves");

  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * (BM + BN) * kRowBytes];
  unsigned char* Xs = smem;                       // [2][BM][kRowBytes]
  unsigned char* Ws = smem + 2 * BM * kRowBytes;  // [2][BN][kRowBytes]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int bm0 = blockIdx.x * BM;
  const int bn0 = blockIdx.y * BN;
  const int cq = tid & 3;     // 16-byte chunk inside the 64-byte k row
  const int lrow = tid >> 2;  // 0..63

  const T* __restrict__ xg = (const T*)a.x;
  const T* __restrict__ wg = (const T*)a.w;

  // ---- per-thread im2col row state (one per pass) ------------------------------------
  int xbase[A_PASSES], hi0[A_PASSES], wi0[A_PASSES];
  bool mok[A_PASSES];
#pragma unroll
  for (int i = 0; i < A_PASSES; ++i) {
    const int r = lrow + 64 * i;
    const int m = bm0 + r;
    mok[i] = (r < BM) && (m < a.M);
    int mm = mok[i] ? m : 0;
    const int wo = mm % a.Wo;
    mm /= a.Wo;
    const int ho = mm % a.Ho;
    const int b = mm / a.Ho;
    hi0[i] = ho * a.SH - a.PT;
    wi0[i] = wo * a.SW - a.PL;
    xbase[i] = ((b * a.H + hi0[i]) * a.W + wi0[i]) * a.x_cs + a.x_co;
  }
  // k state of this thread's chunk
  int kc, kkw, kkh;
  {
    const int kk = cq * EPC;
    kc = kk % a.Cin;
    const int tap = kk / a.Cin;
    kkw = tap % a.KW;
    kkh = tap / a.KW;
  }
  // weight rows
  const T* wrow[B_PASSES];
  bool nok[B_PASSES];
#pragma unroll
  for (int i = 0; i < B_PASSES; ++i) {
    const int r = lrow + 64 * i;
    const int n = bn0 + r;
    nok[i] = (r < BN) && (n < a.Cout);
    wrow[i] = wg + (size_t)(nok[i] ? n : 0) * a.Kpad + cq * EPC;
  }

  const int nk = a.Kpad / BKE;
  uint4 areg[A_PASSES], breg[B_PASSES];
  const uint4 zero4 = make_uint4(0, 0, 0, 0);

  auto load_tile = [&](int kt) {
    const bool kvalid = kkh < a.KH;
    const int koff = (kkh * a.W + kkw) * a.x_cs + kc;
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) {
      const int hi = hi0[i] + kkh, wi = wi0[i] + kkw;
      const bool ok = mok[i] && kvalid && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
      areg[i] = ok ? *(const uint4*)(xg + (xbase[i] + koff)) : zero4;
    }
#pragma unroll
    for (int i = 0; i < B_PASSES; ++i) {
      breg[i] = nok[i] ? *(const uint4*)(wrow[i] + (size_t)kt * BKE) : zero4;
    }
    // advance k state by one tile
    kc += BKE;
    while (kc >= a.Cin) {
      kc -= a.Cin;
      if (++kkw == a.KW) {
        kkw = 0;
        ++kkh;
      }
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) {
      const int r = lrow + 64 * i;
      if (r < BM) *(uint4*)(Xs + (buf * BM + r) * kRowBytes + cq * 16) = areg[i];
    }
#pragma unroll
    for (int i = 0; i < B_PASSES; ++i) {
      const int r = lrow + 64 * i;
      if (r < BN) *(uint4*)(Ws + (buf * BN + r) * kRowBytes + cq * 16) = breg[i];
    }
  };

  f32x4_t acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15, fchunk = lane >> 4;
  const int wbase = (wn * (BN / WN) + frow) * kRowBytes + fchunk * 16;
  const int xbase_l = (wm * (BM / WM) + frow) * kRowBytes + fchunk * 16;
  // n-tiles entirely beyond Cout are skipped (wave-uniform)
  int tn_live = 0;
#pragma unroll
  for (int i = 0; i < TN; ++i)
    if (bn0 + wn * (BN / WN) + i * 16 < a.Cout) tn_live = i + 1;

  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) load_tile(kt + 1);
    uint4 wf[TN], xf[TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
      wf[i] = *(const uint4*)(Ws + buf * BN * kRowBytes + wbase + i * 16 * kRowBytes);
#pragma unroll
    for (int j = 0; j < TM; ++j)
      xf[j] = *(const uint4*)(Xs + buf * BM * kRowBytes + xbase_l + j * 16 * kRowBytes);
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      if (i < tn_live) {
#pragma unroll
        for (int j = 0; j < TM; ++j) {
          if constexpr (sizeof(T) == 2) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                __builtin_bit_cast(bf16x8_t, wf[i]), __builtin_bit_cast(bf16x8_t, xf[j]), acc[i][j], 0, 0, 0);
          } else {
            const f32x4_t wv = __builtin_bit_cast(f32x4_t, wf[i]);
            const f32x4_t xv = __builtin_bit_cast(f32x4_t, xf[j]);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[0], xv[0], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[1], xv[1], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[2], xv[2], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[3], xv[3], acc[i][j], 0, 0, 0);
          }
        }
      }
    }
    if (kt + 1 < nk) store_tile(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue: y = relu(acc * scale[n] + shift[n]) ----------------------------------
  const int mcol = lane & 15, nq = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < TN; ++i) {
    const int n0 = bn0 + wn * (BN / WN) + i * 16 + nq;
    if (n0 >= a.Cout) continue;
    const float4 sc = a.scale ? *(const float4*)(a.scale + n0) : make_float4(1.f, 1.f, 1.f, 1.f);
    const float4 sh = a.scale ? *(const float4*)(a.shift + n0) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      const int m = bm0 + wm * (BM / WM) + j * 16 + mcol;
      if (m >= a.M) continue;
      float v0 = acc[i][j][0] * sc.x + sh.x;
      float v1 = acc[i][j][1] * sc.y + sh.y;
      float v2 = acc[i][j][2] * sc.z + sh.z;
      float v3 = acc[i][j][3] * sc.w + sh.w;
      if (a.relu) {
        v0 = fmaxf(v0, 0.f);
        v1 = fmaxf(v1, 0.f);
        v2 = fmaxf(v2, 0.f);
        v3 = fmaxf(v3, 0.f);
      }
      const size_t off = (size_t)m * a.y_cs + a.y_co + n0;
      if constexpr (MASK) {    // fused activation gradient of the producer conv (ConvArgs::mask_y); T is the plan dtype
        const size_t yoff = (size_t)m * a.mask_cs + a.mask_co + n0;
        float yv[4];
        if (sizeof(T) == 4) {
          const float4 t = *(const float4*)((const float*)a.mask_y + yoff);
          yv[0] = t.x; yv[1] = t.y; yv[2] = t.z; yv[3] = t.w;
        } else {
          const uint2 t = *(const uint2*)((const bf16_t*)a.mask_y + yoff);
          yv[0] = __uint_as_float(t.x << 16); yv[1] = __uint_as_float(t.x & 0xFFFF0000u);
          yv[2] = __uint_as_float(t.y << 16); yv[3] = __uint_as_float(t.y & 0xFFFF0000u);
        }
        const float4 bs = *(const float4*)(a.mask_scale + n0);
        const float g0 = yv[0] > 0.f ? v0 : 0.f, g1 = yv[1] > 0.f ? v1 : 0.f, g2 = yv[2] > 0.f ? v2 : 0.f, g3 = yv[3] > 0.f ? v3 : 0.f;
        float* db = a.mask_dbeta + (size_t)(blockIdx.x & (kMaskCopies - 1)) * a.Cout + n0;
        atomicAdd(db + 0, g0);
        atomicAdd(db + 1, g1);
        atomicAdd(db + 2, g2);
        atomicAdd(db + 3, g3);
        if (sizeof(T) == 4) *(float4*)((float*)a.y + off) = make_float4(g0 * bs.x, g1 * bs.y, g2 * bs.z, g3 * bs.w);
        else *(uint2*)((bf16_t*)a.y + off) = make_uint2(pack_bf16x2(g0 * bs.x, g1 * bs.y), pack_bf16x2(g2 * bs.z, g3 * bs.w));
        continue;
      }
      if (sizeof(T) == 4 || a.out_f32) {
        float4* yp = (float4*)((float*)a.y + off);
        if (a.accum) {
          const float4 o = *yp;
          v0 += o.x; v1 += o.y; v2 += o.z; v3 += o.w;
        }
        *yp = make_float4(v0, v1, v2, v3);
      } else {
        uint2* yp = (uint2*)((bf16_t*)a.y + off);
        if (a.accum) {
          const uint2 o = *yp;
          v0 += __uint_as_float(o.x << 16); v1 += __uint_as_float(o.x & 0xFFFF0000u);
          v2 += __uint_as_float(o.y << 16); v3 += __uint_as_float(o.y & 0xFFFF0000u);
        }
        *yp = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
      }
    }
  }
}

// ---- stem convolution: fp32 NHWC input with Cin <= 4 (images), direct form ------------
// weights fp32 [K = KH*KW*Cin][Cout] staged in LDS; one output pixel per thread, 32 output
// channels per pass.
template <typename T>
__global__ __launch_bounds__(256) void conv_stem_kernel(ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float wsm[];
  const float* __restrict__ wg = (const float*)a.w;
  for (int i = threadIdx.x; i < a.K * a.Cout; i += blockDim.x) wsm[i] = wg[i];
  __syncthreads();
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= a.M) return;
  int mm = pix;
  const int wo = mm % a.Wo;
  mm /= a.Wo;
  const int ho = mm % a.Ho;
  const int b = mm / a.Ho;
  const int hi0 = ho * a.SH - a.PT, wi0 = wo * a.SW - a.PL;
  const float* __restrict__ xg = (const float*)a.x;
  for (int co0 = 0; co0 < a.Cout; co0 += 32) {
    float acc[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) acc[j] = 0.f;
    for (int kh = 0; kh < a.KH; ++kh) {
      const int hi = hi0 + kh;
      if ((unsigned)hi >= (unsigned)a.H) continue;
      for (int kw = 0; kw < a.KW; ++kw) {
        const int wi = wi0 + kw;
        if ((unsigned)wi >= (unsigned)a.W) continue;
        const float* xp = xg + ((size_t)(b * a.H + hi) * a.W + wi) * a.x_cs + a.x_co;
        for (int ci = 0; ci < a.Cin; ++ci) {
          const float xv = xp[ci];
          const float* wr = wsm + ((kh * a.KW + kw) * a.Cin + ci) * a.Cout + co0;
#pragma unroll
          for (int j = 0; j < 32; ++j) acc[j] = fmaf(xv, wr[j], acc[j]);
        }
      }
    }
    const size_t off = (size_t)pix * a.y_cs + a.y_co + co0;
#pragma unroll
    for (int j = 0; j < 32; j += 4) {
      float v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[q] = acc[j + q] * a.scale[co0 + j + q] + a.shift[co0 + j + q];
        if (a.relu) v[q] = fmaxf(v[q], 0.f);
      }
      if (sizeof(T) == 4 || a.out_f32) {
        *(float4*)((float*)a.y + off + j) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        *(uint2*)((bf16_t*)a.y + off + j) = make_uint2(H16<T>::pack(v[0], v[1]), H16<T>::pack(v[2], v[3]));
      }
    }
  }
}

// Stem convolution on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 products, the same
// arithmetic type as the kernel above): K = KH*KW*Cin <= 32 (3x3x3 = 27 -> 7 k-steps of 4), no padding.
// A wave owns 64 consecutive output pixels = 4 column tiles of the swapped product D[cout][pixel];
// the whole filter lives in registers as A fragments, the pixel operand is gathered straight from the
// fp32 image (lane = (pixel, k & 3): 4 consecutive k are (almost always) 4 consecutive floats, and the
// 16 pixels of a tile are SW*Cin floats apart, so a wave load covers a dense span of the image row).
template <typename T, int NT>
__global__ __launch_bounds__(256) void conv_stem_mfma_kernel(ConvArgs a) {
  constexpr int KS = 8;                      // k-steps of 4 (K <= 32)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const float* __restrict__ wg = (const float*)a.w;      // [K][Cout]
  const float* __restrict__ xg = (const float*)a.x;
  // bf16 plans: the 32-deep product runs on the bf16 matrix pipe as hi*hi + hi*lo + lo*hi of the fp32 operands split
  // into two bf16 halves (three 16x16x32 MFMAs of 16 cycles instead of eight fp32 16x16x4 MFMAs of 32: the fp32 form
  // kept the stem matrix-bound at 180 us per 320 images); the dropped lo*lo terms are 2^-16 relative, far below the
  // bf16 rounding of the store.  fp32 plans keep the exact fp32 MFMA.  SPLIT changes the lane -> k map: a lane holds
  // k = 8*fg .. 8*fg+7 (one bf16x8 operand) instead of k = 4*s + fg.
  constexpr bool SPLIT = sizeof(T) == 2;
  float wf[NT][KS];
  int koff[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int k = SPLIT ? 8 * fg + s : 4 * s + fg;
    const bool kv = k < a.K;
    const int kk = kv ? k : 0;
    const int ci = kk % a.Cin, tap = kk / a.Cin;
    const int kw = tap % a.KW, kh = tap / a.KW;
    koff[s] = kv ? (kh * a.W + kw) * a.x_cs + ci : -1;
#pragma unroll
    for (int i = 0; i < NT; ++i) wf[i][s] = kv ? wg[kk * a.Cout + i * 16 + fr] : 0.f;
  }
  // a workgroup walks kStemChunks chunks of 256 pixels with the weight fragments it loaded once
  constexpr int kStemChunks = 4;
  for (int chunk = 0; chunk < kStemChunks; ++chunk) {
  const int pix0 = ((blockIdx.x * kStemChunks + chunk) * 4 + wave) * 64;
  if (pix0 >= a.M) break;
  float xv[4][KS];
  int mrow[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int pix = pix0 + t * 16 + fr;
    const bool ok = pix < a.M;
    int mm = ok ? pix : 0;
    const int wo = mm % a.Wo;
    mm /= a.Wo;
    const int ho = mm % a.Ho;
    const int b = mm / a.Ho;
    const int base = ((b * a.H + ho * a.SH) * a.W + wo * a.SW) * a.x_cs + a.x_co;
    mrow[t] = ok ? pix : -1;
#pragma unroll
    for (int s = 0; s < KS; ++s) xv[t][s] = (ok & (koff[s] >= 0)) ? xg[base + koff[s]] : 0.f;
  }
  f32x4_t acc[NT][4];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[i][t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  if constexpr (SPLIT) {
    auto split8 = [](const float (&v)[KS], bf16x8_t& hi, bf16x8_t& lo) {
      uint32_t h[4], l[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        h[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
        l[e] = pack_bf16x2(v[2 * e] - __uint_as_float(h[e] << 16), v[2 * e + 1] - __uint_as_float(h[e] & 0xFFFF0000u));
      }
      hi = __builtin_bit_cast(bf16x8_t, make_uint4(h[0], h[1], h[2], h[3]));
      lo = __builtin_bit_cast(bf16x8_t, make_uint4(l[0], l[1], l[2], l[3]));
    };
    bf16x8_t wh[NT], wl[NT], xh[4], xl[4];
#pragma unroll
    for (int i = 0; i < NT; ++i) split8(wf[i], wh[i], wl[i]);
#pragma unroll
    for (int t = 0; t < 4; ++t) split8(xv[t], xh[t], xl[t]);
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[i], xh[t], acc[i][t], 0, 0, 0);
        acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[i], xl[t], acc[i][t], 0, 0, 0);
        acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[i], xh[t], acc[i][t], 0, 0, 0);
      }
  } else {
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i][s], xv[t][s], acc[i][t], 0, 0, 0);
  }
  // epilogue: lane holds channels i*16 + fg*4 .. +3 of pixel mrow[t]
  if constexpr (NT == 2 && sizeof(T) == 2) {
    // 32 bf16 channels: the two tiles are exchanged row-wise (see conv_store_tiles) and a lane stores 16 bytes
    if (!a.out_f32 && !a.x3 && (((a.y_cs | a.y_co) & 7) == 0)) {
      float4 sc[2], sh[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        sc[i] = *(const float4*)(a.scale + i * 16 + fg * 4);
        sh[i] = *(const float4*)(a.shift + i * 16 + fg * 4);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        uint32_t pk[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          float v0 = fmaf(acc[i][t][0], sc[i].x, sh[i].x), v1 = fmaf(acc[i][t][1], sc[i].y, sh[i].y);
          float v2 = fmaf(acc[i][t][2], sc[i].z, sh[i].z), v3 = fmaf(acc[i][t][3], sc[i].w, sh[i].w);
          if (a.relu) {
            v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f);
          }
          pk[i][0] = H16<T>::pack(v0, v1);
          pk[i][1] = H16<T>::pack(v2, v3);
        }
        const auto s0 = __builtin_amdgcn_permlane16_swap(pk[0][0], pk[1][0], false, false);
        const auto s1 = __builtin_amdgcn_permlane16_swap(pk[0][1], pk[1][1], false, false);
        if (mrow[t] >= 0)
          *(uint4*)((bf16_t*)a.y + (size_t)mrow[t] * a.y_cs + a.y_co + (fg & 1) * 16 + (fg >> 1) * 8) =
              make_uint4(s0[0], s1[0], s0[1], s1[1]);
      }
      continue;
    }
  }
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int n0 = i * 16 + fg * 4;
    const float4 sc = *(const float4*)(a.scale + n0), sh = *(const float4*)(a.shift + n0);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float v0 = fmaf(acc[i][t][0], sc.x, sh.x), v1 = fmaf(acc[i][t][1], sc.y, sh.y);
      float v2 = fmaf(acc[i][t][2], sc.z, sh.z), v3 = fmaf(acc[i][t][3], sc.w, sh.w);
      if (a.relu) {
        v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f);
      }
      if (mrow[t] < 0) continue;
      const size_t off = (size_t)mrow[t] * a.y_cs + a.y_co + n0;
      if (sizeof(T) == 4 || a.out_f32) {
        *(float4*)((float*)a.y + off) = make_float4(v0, v1, v2, v3);
      } else if (a.x3) {                  // COMIC_OP_X3: [hi | lo | hi] regions
        const uint32_t h01 = pack_bf16x2(v0, v1), h23 = pack_bf16x2(v2, v3);
        const uint32_t l01 = pack_bf16x2(v0 - __uint_as_float(h01 << 16), v1 - __uint_as_float(h01 & 0xFFFF0000u));
        const uint32_t l23 = pack_bf16x2(v2 - __uint_as_float(h23 << 16), v3 - __uint_as_float(h23 & 0xFFFF0000u));
        bf16_t* yp = (bf16_t*)a.y + off;
        *(uint2*)yp = make_uint2(h01, h23);
        *(uint2*)(yp + a.x3) = make_uint2(l01, l23);
        *(uint2*)(yp + 2 * a.x3) = make_uint2(h01, h23);
      } else {
        *(uint2*)((bf16_t*)a.y + off) = make_uint2(H16<T>::pack(v0, v1), H16<T>::pack(v2, v3));
      }
    }
  }
  }
}

// The same product for stems with a LARGE filter and padding (Inception-V1's Conv2d_1a_7x7: 7x7 / stride 2, SAME, 3 -> 64,
// common/nets/inception_v1.py:59-60; K = 147).  The direct kernel above spent 4.3 ms on 640 images (47 % of the
// Inception-V1 forward).  16-bit plans only.
//   * a workgroup owns kStemRows output rows of one image; the input rows they need are staged ONCE in LDS as fp32 with
//     zeroed halo columns / rows (SAME padding costs no per-element test);
//   * k is re-indexed as k' = 24 kh + j, j = kw * Cin + ci < KW * Cin <= 24 (weights of the pad positions are zero): the
//     eight k' of an MFMA operand lane then lie inside ONE filter row, i.e. they are eight consecutive floats of a staged
//     input row -- four ds_read_b64 instead of eight bounds-checked gathers;
//   * every 32-deep chunk runs as hi*hi + hi*lo + lo*hi of bf16 halves; the whole filter lives in registers
//     (KC x NT hi / lo fragment pairs).
constexpr int kStemRows = 2;          // output rows per workgroup
constexpr int kStemKRow = 24;         // k' per filter row
constexpr int kStemFetch = 12;        // float2 a thread moves per staged unit: (rows with weights) * W * Cin / 2 <= 12 * 256
template <typename HT, int NT, int KC>
__global__ __launch_bounds__(256) void conv_stem_wide_kernel(ConvArgs a, int lrow, int blocks_per_image, int total_units) {
  extern __shared__ __attribute__((aligned(16))) float xs[];      // two buffers of [(kStemRows - 1) * SH + 8][lrow]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const float* __restrict__ wg = (const float*)a.w;      // [K][Cout]
  auto split8 = [](const float (&v)[8], bf16x8_t& hi, bf16x8_t& lo) {
    uint32_t h[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      h[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
      l[e] = pack_bf16x2(v[2 * e] - __uint_as_float(h[e] << 16), v[2 * e + 1] - __uint_as_float(h[e] & 0xFFFF0000u));
    }
    hi = __builtin_bit_cast(bf16x8_t, make_uint4(h[0], h[1], h[2], h[3]));
    lo = __builtin_bit_cast(bf16x8_t, make_uint4(l[0], l[1], l[2], l[3]));
  };
  const int nrows = (kStemRows - 1) * a.SH + 8;           // staged rows (filter rows >= KH carry zero weights: never loaded)
  const int lrows = (kStemRows - 1) * a.SH + a.KH;        // ... of which these are loaded
  const int jw = a.KW * a.Cin;                            // floats of one filter row
  const int half = a.W * a.x_cs / 2;                      // float2 per image row (x_cs == Cin: dense NHWC image)
  const float* __restrict__ xg = (const float*)a.x + a.x_co;
  // a unit = kStemRows output rows of one image.  Staged row r = image row ho0*SH - PT + r behind PL*Cin zero floats; rows
  // outside the image are written as zeros, the halo columns are zeroed once and never written again.
  auto fetch = [&](int u, float2 (&v)[kStemFetch]) {
    const int b = u / blocks_per_image, ho0 = (u - b * blocks_per_image) * kStemRows;
#pragma unroll
    for (int q = 0; q < kStemFetch; ++q) {
      const int i = threadIdx.x + 256 * q;
      const int r = i / half, c2 = i - r * half;
      const int hi = ho0 * a.SH - a.PT + r;
      v[q] = make_float2(0.f, 0.f);
      if (r < lrows && (unsigned)hi < (unsigned)a.H) v[q] = *(const float2*)(xg + ((size_t)(b * a.H + hi) * a.W) * a.x_cs + 2 * c2);
    }
  };
  auto stash = [&](float* buf, const float2 (&v)[kStemFetch]) {
#pragma unroll
    for (int q = 0; q < kStemFetch; ++q) {
      const int i = threadIdx.x + 256 * q;
      const int r = i / half, c2 = i - r * half;
      if (r < lrows) *(float2*)(buf + r * lrow + a.PL * a.Cin + 2 * c2) = v[q];
    }
  };
  for (int i = threadIdx.x; i < 2 * nrows * lrow; i += 256) xs[i] = 0.f;
  // ---- the filter as fragments: lane holds k' = 32 c + 8 fg + s of chunk c ------------------------------------------------
  bf16x8_t wh[KC][NT], wl[KC][NT];
  int off[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    const int k0 = 32 * c + 8 * fg;
    const int kh = k0 / kStemKRow, j0 = k0 - kh * kStemKRow;
    off[c] = kh * lrow + j0;
    float wf[NT][8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bool kv = kh < a.KH && j0 + s < jw;
      const int k = kv ? kh * jw + j0 + s : 0;
#pragma unroll
      for (int i = 0; i < NT; ++i) wf[i][s] = kv ? wg[k * a.Cout + i * 16 + fr] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) split8(wf[i], wh[c][i], wl[c][i]);
  }
  // ---- this wave's pixel tiles: tile = wave + 4 t over the kStemRows * Wo pixels of a unit --------------------------------
  const int npix = kStemRows * a.Wo;
  int xbase[4], prow[4], pcol[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int p = (wave + 4 * t) * 16 + fr;
    const int r = p / a.Wo, wo = p - r * a.Wo;
    const bool ok = p < npix;
    xbase[t] = ok ? r * a.SH * lrow + wo * a.SW * a.Cin : 0;
    prow[t] = ok ? r : (1 << 20);
    pcol[t] = wo;
  }
  float2 pre[kStemFetch];
  __syncthreads();                                        // the zero fill is complete
  int unit = blockIdx.x;
  if (unit < total_units) {
    fetch(unit, pre);
    stash(xs, pre);
  }
  __syncthreads();
  for (int it = 0; unit < total_units; unit += gridDim.x, ++it) {
    const float* buf = xs + (it & 1) * nrows * lrow;
    const int next = unit + gridDim.x;
    if (next < total_units) fetch(next, pre);             // in flight under this unit's matrix work
    const int b = unit / blocks_per_image, ho0 = (unit - b * blocks_per_image) * kStemRows;
    f32x4_t acc[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[i][t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      bf16x8_t xh[4], xl[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float2* sp = (const float2*)(buf + xbase[t] + off[c]);      // even float offset: 8-byte aligned
        const float2 v0 = sp[0], v1 = sp[1], v2 = sp[2], v3 = sp[3];
        const float xv[8] = {v0.x, v0.y, v1.x, v1.y, v2.x, v2.y, v3.x, v3.y};
        split8(xv, xh[t], xl[t]);
      }
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[c][i], xh[t], acc[i][t], 0, 0, 0);
          acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[c][i], xl[t], acc[i][t], 0, 0, 0);
          acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[c][i], xh[t], acc[i][t], 0, 0, 0);
        }
    }
    // epilogue: lane holds channels i*16 + fg*4 .. +3 of its pixel of tile t
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int n0 = i * 16 + fg * 4;
      const float4 sc = *(const float4*)(a.scale + n0), sh = *(const float4*)(a.shift + n0);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float v0 = fmaf(acc[i][t][0], sc.x, sh.x), v1 = fmaf(acc[i][t][1], sc.y, sh.y);
        float v2 = fmaf(acc[i][t][2], sc.z, sh.z), v3 = fmaf(acc[i][t][3], sc.w, sh.w);
        if (a.relu) {
          v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f);
        }
        if (ho0 + prow[t] >= a.Ho) continue;
        const size_t o = ((size_t)(b * a.Ho + ho0 + prow[t]) * a.Wo + pcol[t]) * a.y_cs + a.y_co + n0;
        if (a.out_f32)
          *(float4*)((float*)a.y + o) = make_float4(v0, v1, v2, v3);
        else
          *(uint2*)((bf16_t*)a.y + o) = make_uint2(Half16<HT>::pack(v0, v1), Half16<HT>::pack(v2, v3));
      }
    }
    if (next < total_units) stash(xs + ((it + 1) & 1) * nrows * lrow, pre);
    __syncthreads();                                      // the other buffer is complete; this one is free
  }
}

// ---- pooling ---------------------------------------------------------------------------
// MODE 0: max-pool (VALID or padded with -inf)   MODE 1: avg-pool dividing by valid taps
template <typename T, int MODE>
__global__ __launch_bounds__(256) void pool_kernel(ConvArgs a) {
  constexpr int EPC = Elem<T>::EPC;
  const int cvecs = a.Cin / EPC;
  const long total = (long)a.M * cvecs;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int cv = (int)(idx % cvecs);
  int mm = (int)(idx / cvecs);
  const int pix = mm;
  const int wo = mm % a.Wo;
  mm /= a.Wo;
  const int ho = mm % a.Ho;
  const int b = mm / a.Ho;
  const T* __restrict__ xg = (const T*)a.x;
  float acc[EPC];
#pragma unroll
  for (int j = 0; j < EPC; ++j) acc[j] = MODE == 0 ? -INFINITY : 0.f;
  int cnt = 0;
  for (int kh = 0; kh < a.KH; ++kh) {
    const int hi = ho * a.SH - a.PT + kh;
    if ((unsigned)hi >= (unsigned)a.H) continue;
    for (int kw = 0; kw < a.KW; ++kw) {
      const int wi = wo * a.SW - a.PL + kw;
      if ((unsigned)wi >= (unsigned)a.W) continue;
      float v[EPC];
      load_vec<T>(xg + ((size_t)(b * a.H + hi) * a.W + wi) * a.x_cs + a.x_co + cv * EPC, v);
#pragma unroll
      for (int j = 0; j < EPC; ++j) acc[j] = MODE == 0 ? fmaxf(acc[j], v[j]) : acc[j] + v[j];
      ++cnt;
    }
  }
  if (MODE == 1) {
    const float c = (float)cnt;
#pragma unroll
    for (int j = 0; j < EPC; ++j) acc[j] = acc[j] / c;
  }
  store_vec<T>((T*)a.y + (size_t)pix * a.y_cs + a.y_co + cv * EPC, acc);
}

// The same pools over COMIC_OP_X3 buffers: a value is hi + lo of two channel regions.  Max: the pair with the larger hi, then
// the larger lo (|lo| <= ulp(hi) / 2, so this is the order of hi + lo); the winning pair is copied.  Average: fp32 sum of
// hi + lo over the valid taps, divided, split again.  Output: the three regions [hi | lo | hi].
template <int MODE>
__global__ __launch_bounds__(256) void pool_x3_kernel(ConvArgs a) {
  constexpr int EPC = 8;
  const int cvecs = a.Cin / EPC;
  const long total = (long)a.M * cvecs;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int cv = (int)(idx % cvecs);
  int mm = (int)(idx / cvecs);
  const int pix = mm;
  const int wo = mm % a.Wo;
  mm /= a.Wo;
  const int ho = mm % a.Ho;
  const int b = mm / a.Ho;
  const bf16_t* __restrict__ xg = (const bf16_t*)a.x;
  float hi[EPC], lo[EPC];
#pragma unroll
  for (int j = 0; j < EPC; ++j) {
    hi[j] = MODE == 0 ? -INFINITY : 0.f;
    lo[j] = 0.f;
  }
  int cnt = 0;
  for (int kh = 0; kh < a.KH; ++kh) {
    const int hy = ho * a.SH - a.PT + kh;
    if ((unsigned)hy >= (unsigned)a.H) continue;
    for (int kw = 0; kw < a.KW; ++kw) {
      const int wx = wo * a.SW - a.PL + kw;
      if ((unsigned)wx >= (unsigned)a.W) continue;
      float vh[EPC], vl[EPC];
      const bf16_t* src = xg + ((size_t)(b * a.H + hy) * a.W + wx) * a.x_cs + a.x_co + cv * EPC;
      load_vec<bf16_t>(src, vh);
      load_vec<bf16_t>(src + a.x3_src, vl);
#pragma unroll
      for (int j = 0; j < EPC; ++j) {
        if (MODE == 0) {
          const bool take = vh[j] > hi[j] || (vh[j] == hi[j] && vl[j] > lo[j]);
          hi[j] = take ? vh[j] : hi[j];
          lo[j] = take ? vl[j] : lo[j];
        } else {
          hi[j] += vh[j] + vl[j];
        }
      }
      ++cnt;
    }
  }
  if (MODE == 1) {
    const float c = (float)cnt;
#pragma unroll
    for (int j = 0; j < EPC; ++j) {
      const float v = hi[j] / c;
      hi[j] = bf16_to_f32(f32_to_bf16(v));
      lo[j] = v - hi[j];
    }
  }
  bf16_t* dst = (bf16_t*)a.y + (size_t)pix * a.y_cs + a.y_co + cv * EPC;
  store_vec<bf16_t>(dst, hi);
  store_vec<bf16_t>(dst + a.x3, lo);
  store_vec<bf16_t>(dst + 2 * a.x3, hi);
}

// 3x3 stride-1 SAME max-pool (the pool branches of the Inception-V1 / V3 blocks) as one thread per (image row, channel
// vector): the thread walks the row and keeps the maxima of the last three columns over the (up to three) valid source
// rows, so every source element is loaded once per output ROW that needs it (3 loads per output instead of 9; the
// generic kernel above took 22 % of the Inception-V1 forward).  max is exact in any order: same results.
template <typename T>
__global__ __launch_bounds__(256) void maxpool3_rows_kernel(ConvArgs a) {
  constexpr int EPC = Elem<T>::EPC;
  const int cvecs = a.Cin / EPC;
  const long total = (long)a.B * a.H * cvecs;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int cv = (int)(idx % cvecs);
  const int q = (int)(idx / cvecs);
  const int ho = q % a.H, b = q / a.H;
  const T* __restrict__ xg = (const T*)a.x;
  const int r0 = max(ho - 1, 0), r1 = min(ho + 1, a.H - 1);
  auto colmax = [&](int w, float (&m)[EPC]) {
#pragma unroll
    for (int j = 0; j < EPC; ++j) m[j] = -INFINITY;
    for (int r = r0; r <= r1; ++r) {
      float v[EPC];
      load_vec<T>(xg + ((size_t)(b * a.H + r) * a.W + w) * a.x_cs + a.x_co + cv * EPC, v);
#pragma unroll
      for (int j = 0; j < EPC; ++j) m[j] = fmaxf(m[j], v[j]);
    }
  };
  float c0[EPC], c1[EPC], c2[EPC];
#pragma unroll
  for (int j = 0; j < EPC; ++j) c0[j] = -INFINITY;
  colmax(0, c1);
  for (int wo = 0; wo < a.W; ++wo) {
    if (wo + 1 < a.W) {
      colmax(wo + 1, c2);
    } else {
#pragma unroll
      for (int j = 0; j < EPC; ++j) c2[j] = -INFINITY;
    }
    float o[EPC];
#pragma unroll
    for (int j = 0; j < EPC; ++j) o[j] = fmaxf(fmaxf(c0[j], c1[j]), c2[j]);
    store_vec<T>((T*)a.y + ((size_t)(b * a.H + ho) * a.W + wo) * a.y_cs + a.y_co + cv * EPC, o);
#pragma unroll
    for (int j = 0; j < EPC; ++j) {
      c0[j] = c1[j];
      c1[j] = c2[j];
    }
  }
}

// 16-bit store of four channels of a kind-7 output; a.x3 (COMIC_OP_X3, bf16 plans): as the three regions [hi | lo | hi]
template <typename HT>
__device__ __forceinline__ void pbr_store_16(const ConvArgs& a, size_t off, float v0, float v1, float v2, float v3) {
  bf16_t* yp = (bf16_t*)a.y + off;
  const uint32_t h01 = Half16<HT>::pack(v0, v1), h23 = Half16<HT>::pack(v2, v3);
  *(uint2*)yp = make_uint2(h01, h23);
  if (a.x3) {
    const uint32_t l01 = pack_bf16x2(v0 - __uint_as_float(h01 << 16), v1 - __uint_as_float(h01 & 0xFFFF0000u));
    const uint32_t l23 = pack_bf16x2(v2 - __uint_as_float(h23 << 16), v3 - __uint_as_float(h23 & 0xFFFF0000u));
    *(uint2*)(yp + a.x3) = make_uint2(l01, l23);
    *(uint2*)(yp + 2 * a.x3) = make_uint2(h01, h23);
  }
}

// kind 7: 3x3 s1 SAME average (divisor = taps inside the image) of an fp32 map, then the folded
// BatchNorm + ReLU of the projection that produced it.  One thread per (pixel, 4 channels).
template <typename HT>
__device__ __forceinline__ void pool_bn_relu_item(const ConvArgs& a, const long idx, const int cvecs) {
  const int cv = (int)(idx % cvecs);
  int mm = (int)(idx / cvecs);
  const int pix = mm;
  const int wo = mm % a.Wo;
  mm /= a.Wo;
  const int ho = mm % a.Ho;
  const int b = mm / a.Ho;
  const float* __restrict__ xg = (const float*)a.x;
  // all nine taps are loaded unconditionally from clamped coordinates (nine independent 16-byte loads in flight);
  // taps outside the image are then skipped in the sum, in the same (kh, kw) order as a branchy loop
  float4 v[9];
  bool ok[9];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int hi = ho - 1 + kh;
    const int hc = min(max(hi, 0), a.H - 1);
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int wi = wo - 1 + kw;
      const int wc = min(max(wi, 0), a.W - 1);
      ok[kh * 3 + kw] = ((unsigned)hi < (unsigned)a.H) & ((unsigned)wi < (unsigned)a.W);
      v[kh * 3 + kw] = *(const float4*)(xg + ((size_t)(b * a.H + hc) * a.W + wc) * a.x_cs + a.x_co + cv * 4);
    }
  }
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int cnt = 0;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    if (ok[t]) {
      acc.x += v[t].x; acc.y += v[t].y; acc.z += v[t].z; acc.w += v[t].w;
      ++cnt;
    }
  }
  const float c = (float)cnt;
  const float4 sc = *(const float4*)(a.scale + cv * 4), sh = *(const float4*)(a.shift + cv * 4);
  float v0 = acc.x / c * sc.x + sh.x, v1 = acc.y / c * sc.y + sh.y, v2 = acc.z / c * sc.z + sh.z, v3 = acc.w / c * sc.w + sh.w;
  if (a.relu) {
    v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f);
  }
  const size_t off = (size_t)pix * a.y_cs + a.y_co + cv * 4;
  if (a.out_f32)
    *(float4*)((float*)a.y + off) = make_float4(v0, v1, v2, v3);
  else
    pbr_store_16<HT>(a, off, v0, v1, v2, v3);
}

template <typename HT>
__global__ __launch_bounds__(256) void pool_bn_relu_kernel(ConvArgs a) {
  const int cvecs = a.Cin / 4;
  const long total = (long)a.M * cvecs;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < total) pool_bn_relu_item<HT>(a, idx, cvecs);
}

// The same op as one thread per (image row, 4 channels): the thread walks the row and keeps the sums of the last three
// columns over the (up to three) valid source rows, so every source element is loaded once per output ROW that needs it
// (3 loads per output instead of 9).  Summation order: rows inside a column first, then the columns left to right.
template <typename HT>
__global__ __launch_bounds__(256) void pool_bn_relu_rows_kernel(ConvArgs a) {
  const int cvecs = a.Cin / 4;
  const long total = (long)a.B * a.H * cvecs;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int cv = (int)(idx % cvecs);
  const int q = (int)(idx / cvecs);
  const int ho = q % a.H, b = q / a.H;
  const float* __restrict__ xg = (const float*)a.x;
  const int r0 = max(ho - 1, 0), r1 = min(ho + 1, a.H - 1);
  const float nrows = (float)(r1 - r0 + 1);
  const float4 sc = *(const float4*)(a.scale + cv * 4), sh = *(const float4*)(a.shift + cv * 4);
  const float lo = a.relu ? 0.f : -INFINITY;
  // The row is walked in blocks of kAhead columns whose source loads are all issued before the first of them is used: with
  // the loads of column wo + 1 requested in the iteration that consumes them, every output pixel waited a full memory
  // round trip (84 us for 1280 x 25 x 25 x 64: twice the HBM floor).  Same sums in the same order.
  constexpr int kAhead = 4;
  auto col_loads = [&](int w, float4 (&v)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int r = r0 + k;
      v[k] = (w < a.W && r <= r1) ? *(const float4*)(xg + ((size_t)(b * a.H + r) * a.W + w) * a.x_cs + a.x_co + cv * 4)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto col_sum = [&](const float4 (&v)[3]) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (r0 + k <= r1) { s.x += v[k].x; s.y += v[k].y; s.z += v[k].z; s.w += v[k].w; }
    return s;
  };
  float4 c0 = make_float4(0.f, 0.f, 0.f, 0.f), c1, c2;
  {
    float4 v[3];
    col_loads(0, v);
    c1 = col_sum(v);
  }
  for (int w0 = 0; w0 < a.W; w0 += kAhead) {
    float4 nx[kAhead][3];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) col_loads(w0 + u + 1, nx[u]);      // columns w0 + 1 .. w0 + kAhead (zeros past the row)
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const int wo = w0 + u;
      if (wo >= a.W) break;
      const bool right = wo + 1 < a.W;
      c2 = right ? col_sum(nx[u]) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float cnt = nrows * (float)(1 + (wo > 0) + right);
      float v0 = ((c0.x + c1.x) + c2.x) / cnt * sc.x + sh.x, v1 = ((c0.y + c1.y) + c2.y) / cnt * sc.y + sh.y;
      float v2 = ((c0.z + c1.z) + c2.z) / cnt * sc.z + sh.z, v3 = ((c0.w + c1.w) + c2.w) / cnt * sc.w + sh.w;
      v0 = fmaxf(v0, lo); v1 = fmaxf(v1, lo); v2 = fmaxf(v2, lo); v3 = fmaxf(v3, lo);
      const size_t off = ((size_t)(b * a.H + ho) * a.W + wo) * a.y_cs + a.y_co + cv * 4;
      if (a.out_f32)
        *(float4*)((float*)a.y + off) = make_float4(v0, v1, v2, v3);
      else
        pbr_store_16<HT>(a, off, v0, v1, v2, v3);
      c0 = c1;
      c1 = c2;
    }
  }
}

// The same work as a member of a grouped conv launch: workgroup `local` of this member handles
// kPoolItemsPerThread x blockDim.x consecutive (pixel, 4-channel) items.
constexpr int kPoolItemsPerThread = 4;
template <typename HT>
__device__ __forceinline__ void pool_bn_relu_member(const ConvArgs& a, const int local) {
  const int cvecs = a.Cin / 4;
  const long total = (long)a.M * cvecs;
  const long base = (long)local * blockDim.x * kPoolItemsPerThread + threadIdx.x;
#pragma unroll
  for (int r = 0; r < kPoolItemsPerThread; ++r) {
    const long idx = base + (long)r * blockDim.x;
    if (idx < total) pool_bn_relu_item<HT>(a, idx, cvecs);
  }
}

// global KHxKW VALID average -> fp32 [B, Ho*Wo, C]; one thread per (pixel, channel vec)
template <typename T>
__global__ __launch_bounds__(256) void global_avgpool_kernel(ConvArgs a) {
  constexpr int EPC = Elem<T>::EPC;
  const int cvecs = a.Cin / EPC;
  const long total = (long)a.M * cvecs;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int cv = (int)(idx % cvecs);
  int mm = (int)(idx / cvecs);
  const int pix = mm;
  const int wo = mm % a.Wo;
  mm /= a.Wo;
  const int ho = mm % a.Ho;
  const int b = mm / a.Ho;
  const T* __restrict__ xg = (const T*)a.x;
  float acc[EPC];
#pragma unroll
  for (int j = 0; j < EPC; ++j) acc[j] = 0.f;
  for (int kh = 0; kh < a.KH; ++kh)
    for (int kw = 0; kw < a.KW; ++kw) {
      float v[EPC];
      load_vec<T>(xg + ((size_t)(b * a.H + ho * a.SH + kh) * a.W + wo * a.SW + kw) * a.x_cs + a.x_co + cv * EPC, v);
#pragma unroll
      for (int j = 0; j < EPC; ++j) acc[j] += v[j];
    }
  const float inv = (float)(a.KH * a.KW);
  float* yp = (float*)a.y + (size_t)pix * a.y_cs + a.y_co + cv * EPC;
#pragma unroll
  for (int j = 0; j < EPC; ++j) yp[j] = acc[j] / inv;
}

// ---- weight packing / BN folding -----------------------------------------------------------
template <typename T>
__global__ void pack_conv_weights_kernel(const float* __restrict__ w, T* __restrict__ out, int K, int Kpad,
                                         int cout) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)cout * Kpad) return;
  const int k = (int)(idx % Kpad), n = (int)(idx / Kpad);
  const float v = k < K ? w[(size_t)k * cout + n] : 0.f;
  if (sizeof(T) == 4)
    ((float*)out)[idx] = v;
  else
    ((typename Half16Of<T>::type*)out)[idx] = H16<T>::from_f32(v);
}

__global__ void fold_bn_kernel(const float* beta, const float* mean, const float* var, float eps, float* scale,
                               float* shift, int c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c) return;
  const float s = 1.0f / sqrtf(var[i] + eps);
  scale[i] = s;
  shift[i] = beta[i] - mean[i] * s;
}


// ---------------------------------------------------------------------------------------------
// bf16 throughput path: LDS-DMA pipelined implicit GEMM.
//
// Same math and orientation as conv_igemm_kernel, but the operand tiles go global -> LDS with
// `global_load_lds_dwordx4` (no VGPR staging) into a ring of NSTAGE stages of [rows][128 B of
// k] (BK = 64 bf16), so two whole k-tiles stay in flight behind the one being multiplied.
// One raw s_barrier per k-tile; DMA completion is tracked with counted `s_waitcnt vmcnt(N)`;
// fragment reads are inline-asm ds_read_b128 (hipcc would otherwise drain vmcnt(0) in front of
// every LDS read that may alias an in-flight DMA -- cdna_hip_programming.md §5).
//
// LDS image: 128-byte rows, 16-byte slot = chunk ^ ((row >> 1) & 7).  The DMA writes LDS
// linearly (wave base + lane*16), so the swizzle is applied to the per-lane SOURCE chunk; the
// ds_read_b128 lane groups of the 16x16x32 operand fetch then hit 16 distinct slots.
// Padding / out-of-range rows read from a 16-byte zero page.
__device__ __attribute__((aligned(16))) unsigned int g_zero_page[4] = {0u, 0u, 0u, 0u};


// ALIGNED (Cin % 64 == 0): a whole k-tile lies inside one filter tap, so the tap walk (kh, kw, c0)
// is wave-uniform scalar state and the per-lane part of a source address is a constant.
// NSTAGE_ = kLoaderWaves + n: n ring stages and WAVE SPECIALISATION -- the WM x WN waves only read fragments and issue
// MFMAs, four more waves only issue the LDS-DMA pieces.  An LDS-DMA instruction holds its wave for ~70 cycles (stamps:
// 700 of the 1950 cycles of a 128x192 k-tile went into issuing its 10 pieces); on a wave of its own that time runs
// beside the matrix work instead of in front of it.  Both roles execute one s_barrier per k-tile.
constexpr int kLoaderWaves = 20;
constexpr int ring_stages(int nstage) { return nstage % 10; }
constexpr int dma_threads(int wm, int wn, int nstage) { return (wm * wn + (nstage >= kLoaderWaves ? 4 : 0)) * 64; }

template <typename HT, int BM, int BN, int WM, int WN, int NSTAGE_, bool ALIGNED, bool MASK = false>
__device__ __forceinline__ void conv_igemm_dma_body(const ConvArgs& a, const int block_m, const int block_n) {
  constexpr int BKE = 64;                       // bf16 elements per k-tile = 128 bytes per row
  constexpr int ROWS = BM + BN;
  constexpr int STAGE_BYTES = ROWS * 128;
  constexpr int NSTAGE = ring_stages(NSTAGE_);
  constexpr bool SPEC = NSTAGE_ >= kLoaderWaves;
  constexpr int NWC = WM * WN;                  // waves that own output tiles (4 or 8)
  constexpr int NW = SPEC ? 4 : NWC;            // waves that issue the LDS-DMA pieces
  constexpr int IPW_A = BM / (8 * NW);          // 8-row DMA instructions per wave per stage (A)
  constexpr int IPW_B = BN / (8 * NW);
  constexpr int LPT = IPW_A + IPW_B;            // DMA instructions per wave per stage
  constexpr int TM = BM / WM / 16;
  constexpr int TN = BN / WN / 16;
  static_assert((NWC == 4 || NWC == 8) && BM % (8 * NW) == 0 && BN % (8 * NW) == 0 && BM % (16 * WM) == 0 &&
                    BN % (16 * WN) == 0, "tile shape");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) unsigned char*)smem);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave_id = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: LDS DMA bases become SGPR math
  const bool loader = SPEC && wave_id >= NWC;
  const int wave = loader ? wave_id - NWC : wave_id;           // index inside its role
  const int wm = wave / WN, wn = wave % WN;
  const int bm0 = block_m * BM, bn0 = block_n * BN;
  const bf16_t* __restrict__ xg = (const bf16_t*)a.x;
  const bf16_t* __restrict__ wg = (const bf16_t*)a.w;
  const bf16_t* zp = (const bf16_t*)a.zero;
  const int slot = lane & 7, rsub = lane >> 3;

  // ---- im2col state of the rows this lane feeds ------------------------------------------
  int xbase[IPW_A], hi0[IPW_A], wi0[IPW_A];
  bool mok[IPW_A];
#pragma unroll
  for (int i = 0; i < IPW_A; ++i) {
    const int r = (wave * IPW_A + i) * 8 + rsub;
    const int m = bm0 + r;
    mok[i] = m < a.M;
    int mm = mok[i] ? m : 0;
    const int wo = mm % a.Wo;
    mm /= a.Wo;
    const int ho = mm % a.Ho;
    const int b = mm / a.Ho;
    hi0[i] = ho * a.SH - a.PT;
    wi0[i] = wo * a.SW - a.PL;
    xbase[i] = ((b * a.H + hi0[i]) * a.W + wi0[i]) * a.x_cs + a.x_co;
  }
  // the source chunk of a lane alternates between two values with the parity of the 8-row group
  // (swizzle term (row>>1)&7 = 4*(group&1) + (rsub>>1)); keep one k-state per parity
  int kc[2], kkw[2], kkh[2];
  int chunk8[2];          // ALIGNED: element offset of this lane's chunk inside the k-tile, per parity
  int s_kh = 0, s_kw = 0, s_c0 = 0;   // ALIGNED: wave-uniform tap walk
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int chunk = slot ^ ((4 * par + (rsub >> 1)) & 7);
    const int kk = chunk * 8;
    chunk8[par] = kk;
    kc[par] = kk % a.Cin;
    const int tap = kk / a.Cin;
    kkw[par] = tap % a.KW;
    kkh[par] = tap / a.KW;
  }
  const bf16_t* wsrc[IPW_B];
  bool nok[IPW_B];
#pragma unroll
  for (int i = 0; i < IPW_B; ++i) {
    const int gb = wave * IPW_B + i;
    const int n = bn0 + gb * 8 + rsub;
    nok[i] = n < a.Cout;
    const int chunk = slot ^ ((4 * (gb & 1) + (rsub >> 1)) & 7);
    wsrc[i] = wg + (size_t)(nok[i] ? n : 0) * a.Kpad + chunk * 8;
  }
  const int nk = a.Kpad / BKE;

  auto issue = [&](int kt, int stage) {
    unsigned char* sbase = smem + stage * STAGE_BYTES;
    if constexpr (ALIGNED) {
      const bool kvalid = s_kh < a.KH;
      const int koff = (s_kh * a.W + s_kw) * a.x_cs + s_c0;   // scalar
#pragma unroll
      for (int i = 0; i < IPW_A; ++i) {
        const int ga = wave * IPW_A + i;
        const int hi = hi0[i] + s_kh, wi = wi0[i] + s_kw;
        const bool ok = mok[i] & kvalid & ((unsigned)hi < (unsigned)a.H) & ((unsigned)wi < (unsigned)a.W);
        const bf16_t* src = xg + (xbase[i] + koff + chunk8[ga & 1]);
        src = ok ? src : zp;
        dma16(src, sbase + ga * 1024);
      }
    } else {
#pragma unroll
      for (int i = 0; i < IPW_A; ++i) {
        const int ga = wave * IPW_A + i;
        const int par = ga & 1;
        const int hi = hi0[i] + kkh[par], wi = wi0[i] + kkw[par];
        const bool ok = mok[i] & (kkh[par] < a.KH) & ((unsigned)hi < (unsigned)a.H) & ((unsigned)wi < (unsigned)a.W);
        const bf16_t* src = xg + (xbase[i] + (kkh[par] * a.W + kkw[par]) * a.x_cs + kc[par]);
        src = ok ? src : zp;
        dma16(src, sbase + ga * 1024);
      }
    }
#pragma unroll
    for (int i = 0; i < IPW_B; ++i) {
      const int gb = wave * IPW_B + i;
      const bf16_t* src = wsrc[i] + (size_t)kt * BKE;
      src = nok[i] ? src : zp;
      dma16(src, sbase + BM * 128 + gb * 1024);
    }
    if constexpr (ALIGNED) {
      s_c0 += BKE;
      if (s_c0 >= a.Cin) {
        s_c0 = 0;
        if (++s_kw == a.KW) {
          s_kw = 0;
          ++s_kh;
        }
      }
    } else {
#pragma unroll
      for (int par = 0; par < 2; ++par) {
        kc[par] += BKE;
        while (kc[par] >= a.Cin) {
          kc[par] -= a.Cin;
          if (++kkw[par] == a.KW) {
            kkw[par] = 0;
            ++kkh[par];
          }
        }
      }
    }
  };

  f32x4_t acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  // fragment addressing: lane (r, g) reads row r of a 16-row tile, k-chunk ks*4+g, at slot chunk^((r>>1)&7)
  const int fr = lane & 15, fg = lane >> 4;
  const uint32_t sw = (fr >> 1) & 7;
  const uint32_t x_off0 = (wm * (BM / WM) + fr) * 128 + (((0 + fg) ^ sw) & 7) * 16;
  const uint32_t x_off1 = (wm * (BM / WM) + fr) * 128 + (((4 + fg) ^ sw) & 7) * 16;
  const uint32_t w_off0 = (BM + wn * (BN / WN) + fr) * 128 + (((0 + fg) ^ sw) & 7) * 16;
  const uint32_t w_off1 = (BM + wn * (BN / WN) + fr) * 128 + (((4 + fg) ^ sw) & 7) * 16;

  // NSTAGE-1 tiles are in flight before the loop; at the top of iteration kt the tiles
  // kt .. min(kt+NSTAGE-2, nk-1) have been issued and tile kt must have landed.
  constexpr int AHEAD = NSTAGE - 1;
  STAMP(0);
  if constexpr (SPEC) {
    if (loader) {
      // loader waves: keep AHEAD tiles in flight; tile kt must have landed before barrier kt releases its readers
#pragma unroll
      for (int p = 0; p < AHEAD; ++p)
        if (p < nk) issue(p, p);
      for (int kt = 0; kt < nk; ++kt) {
        const int pending = min(AHEAD - 1, nk - 1 - kt);
        if (pending >= 2)
          wait_vmcnt<2 * LPT>();
        else if (pending == 1)
          wait_vmcnt<LPT>();
        else
          wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (kt + AHEAD < nk) issue(kt + AHEAD, (kt + AHEAD) % NSTAGE);
      }
      return;
    }
  } else {
#pragma unroll
    for (int p = 0; p < AHEAD; ++p)
      if (p < nk) issue(p, p);
  }
  STAMP(1);
#ifdef COMIC_STAMPS
  unsigned long long t_issue = 0, t_wait = 0;
#endif
  for (int kt = 0; kt < nk; ++kt) {
    const int stage = kt % NSTAGE;
#ifdef COMIC_STAMPS
    const unsigned long long tw0 = __builtin_amdgcn_s_memtime();
#endif
    if constexpr (!SPEC) {
      const int pending = min(AHEAD - 1, nk - 1 - kt);   // tiles allowed to stay in flight
      if (pending >= 2)
        wait_vmcnt<2 * LPT>();
      else if (pending == 1)
        wait_vmcnt<LPT>();
      else
        wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();   // every wave's share of tile kt landed; the stage read in kt-1 is free
#ifdef COMIC_STAMPS
    const unsigned long long ti0 = __builtin_amdgcn_s_memtime();
    t_wait += ti0 - tw0;
    if (kt == 0 && tid == 0) g_stamps[(blockIdx.x & 16383) * 8 + 7] = ti0 - tw0;    // the wait for the FIRST k-tile
#endif
    if constexpr (!SPEC) {
      if (kt + AHEAD < nk) issue(kt + AHEAD, (kt + AHEAD) % NSTAGE);
    }
#ifdef COMIC_STAMPS
    t_issue += __builtin_amdgcn_s_memtime() - ti0;
#endif
    const uint32_t sb = lds0 + stage * STAGE_BYTES;
    u32x4_t xf0[TM], xf1[TM], wf0[TN], wf1[TN];
    // both 32-deep halves of the k-tile are requested at once; the first half's MFMAs start as soon as ITS fragments
    // have landed (the LDS returns in order: lgkmcnt <= TM+TN leaves exactly the second half outstanding), so the
    // second half's read latency runs under them.  Per accumulator the order stays half 0, then half 1.
    static_assert(TM + TN <= 15, "lgkmcnt holds 4 bits");
    static_for<0, TN>([&](auto i) { wf0[i] = lds_read128<decltype(i)::value * 2048>(sb + w_off0); });
    static_for<0, TM>([&](auto j) { xf0[j] = lds_read128<decltype(j)::value * 2048>(sb + x_off0); });
    static_for<0, TN>([&](auto i) { wf1[i] = lds_read128<decltype(i)::value * 2048>(sb + w_off1); });
    static_for<0, TM>([&](auto j) { xf1[j] = lds_read128<decltype(j)::value * 2048>(sb + x_off1); });
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(TM + TN) : "memory");
    __builtin_amdgcn_sched_barrier(0);
    // n-tiles beyond Cout multiply zero-filled weight rows (no branch: keeps the accumulators in place)
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j)
        acc[i][j] = Half16<HT>::mfma(__builtin_bit_cast(bf16x8_t, wf0[i]),
                                                            __builtin_bit_cast(bf16x8_t, xf0[j]), acc[i][j]);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j)
        acc[i][j] = Half16<HT>::mfma(__builtin_bit_cast(bf16x8_t, wf1[i]),
                                                            __builtin_bit_cast(bf16x8_t, xf1[j]), acc[i][j]);
  }

  STAMP(2);
#ifdef COMIC_STAMPS
  if (tid == 0) { g_stamps[(blockIdx.x & 16383) * 8 + 4] = t_issue; g_stamps[(blockIdx.x & 16383) * 8 + 5] = t_wait; g_stamps[(blockIdx.x & 16383) * 8 + 6] = nk; }
#endif
  // ---- epilogue: y = relu(acc * scale[n] + shift[n]) ----------------------------------
  int mrow[TM];
#pragma unroll
  for (int j = 0; j < TM; ++j) {
    const int m = bm0 + wm * (BM / WM) + j * 16 + (lane & 15);
    mrow[j] = m < a.M ? m : -1;
  }
  conv_store_tiles<HT, TN, TM, MASK>(a, acc, bn0 + wn * (BN / WN), (lane >> 4) * 4, mrow);
  STAMP(3);
}



// ---------------------------------------------------------------------------------------------
// "Walk" form of the loader-wave kernel for launches whose members read the SAME im2col matrix (the 1x1 convs at the head
// of an Inception block; ConvArgs::remap == 3): ONE workgroup per pixel tile walks over the out-channel tiles of ALL
// members.  Why (phase stamps of the 12x12 768 -> 704 groups at 1280 images, one tile per workgroup): the wait for the first
// k-tile is 14 % of a workgroup's life, 43 % of the k loop is spent at the barrier waiting for rows that come from HBM again
// although three sibling workgroups fetch the same rows (L2 hit rate of the pixel operand 0.54), the epilogue another 14 %.
// Here the k-tile stream of the loader waves runs on across the out-channel tiles (the ring never drains: the first
// k-tiles of the next tile land under the epilogue of this one), and after the first tile the pixel rows come from the
// L2 this workgroup has just filled.  Same operands in the same order per accumulator as conv_igemm_dma_body: identical bits.
template <typename HT, int BM, int BN, int WM, int WN, int NSTAGE_, bool ALIGNED>
__device__ __forceinline__ void conv_igemm_dma_walk_body(const ConvArgs* __restrict__ args, const int n_members, const int block_m,
                                                         const int r_begin, const int r_end) {   // out-channel tiles [r_begin, r_end) of the walk
  constexpr int BKE = 64;
  constexpr int ROWS = BM + BN;
  constexpr int STAGE_BYTES = ROWS * 128;
  constexpr int NSTAGE = ring_stages(NSTAGE_);
  static_assert(NSTAGE_ >= kLoaderWaves, "the walk form needs the loader waves");
  constexpr int NWC = WM * WN;
  constexpr int NW = 4;
  constexpr int IPW_A = BM / (8 * NW);
  constexpr int IPW_B = BN / (8 * NW);
  constexpr int LPT = IPW_A + IPW_B;
  constexpr int TM = BM / WM / 16;
  constexpr int TN = BN / WN / 16;
  constexpr int AHEAD = NSTAGE - 1;
  static_assert(NWC == 4 && BM % (8 * NW) == 0 && BN % (8 * NW) == 0 && BM % (16 * WM) == 0 && BN % (16 * WN) == 0, "tile shape");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) unsigned char*)smem);
  const ConvArgs& a = args[0];                   // everything about the pixel operand is common to the members
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave_id = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool loader = wave_id >= NWC;
  const int wave = loader ? wave_id - NWC : wave_id;
  const int wm = wave / WN, wn = wave % WN;
  const int bm0 = block_m * BM;
  const int nk = a.Kpad / BKE;
  const int total = (r_end - r_begin) * nk;      // k-tiles of the whole walk
  const int slot = lane & 7, rsub = lane >> 3;

  if (loader) {
    const bf16_t* __restrict__ xg = (const bf16_t*)a.x;
    const bf16_t* zp = (const bf16_t*)a.zero;
    int xbase[IPW_A], hi0[IPW_A], wi0[IPW_A];
    bool mok[IPW_A];
#pragma unroll
    for (int i = 0; i < IPW_A; ++i) {
      const int r = (wave * IPW_A + i) * 8 + rsub;
      const int m = bm0 + r;
      mok[i] = m < a.M;
      int mm = mok[i] ? m : 0;
      const int wo = mm % a.Wo;
      mm /= a.Wo;
      const int ho = mm % a.Ho;
      const int b = mm / a.Ho;
      hi0[i] = ho * a.SH - a.PT;
      wi0[i] = wo * a.SW - a.PL;
      xbase[i] = ((b * a.H + hi0[i]) * a.W + wi0[i]) * a.x_cs + a.x_co;
    }
    int kc[2], kkw[2], kkh[2], chunk8[2];
    int s_kh = 0, s_kw = 0, s_c0 = 0;
    auto reset_k = [&]() {
      s_kh = s_kw = s_c0 = 0;
#pragma unroll
      for (int par = 0; par < 2; ++par) {
        const int chunk = slot ^ ((4 * par + (rsub >> 1)) & 7);
        const int kk = chunk * 8;
        chunk8[par] = kk;
        kc[par] = kk % a.Cin;
        const int tap = kk / a.Cin;
        kkw[par] = tap % a.KW;
        kkh[par] = tap / a.KW;
      }
    };
    const bf16_t* wsrc[IPW_B];
    bool nok[IPW_B];
    auto set_tile = [&](int r) {                 // weight rows of out-channel tile r (member p, its tile r - blk0)
      int p = 0;
      for (int i = 1; i < n_members; ++i)
        if (r >= args[i].blk0) p = i;
      const bf16_t* wg = (const bf16_t*)args[p].w;
      const int bn0 = (r - args[p].blk0) * BN, cout = args[p].Cout;
#pragma unroll
      for (int i = 0; i < IPW_B; ++i) {
        const int gb = wave * IPW_B + i;
        const int nn = bn0 + gb * 8 + rsub;
        nok[i] = nn < cout;
        const int chunk = slot ^ ((4 * (gb & 1) + (rsub >> 1)) & 7);
        wsrc[i] = wg + (size_t)(nok[i] ? nn : 0) * a.Kpad + chunk * 8;
      }
    };
    int gi = 0, gi_kt = 0, gi_r = r_begin;       // issue pointer: stream index, its k-tile and out-channel tile
    auto issue = [&]() {
      if (gi_kt == 0) {
        set_tile(gi_r);
        reset_k();
      }
      unsigned char* sbase = smem + (gi % NSTAGE) * STAGE_BYTES;
      if constexpr (ALIGNED) {
        const bool kvalid = s_kh < a.KH;
        const int koff = (s_kh * a.W + s_kw) * a.x_cs + s_c0;
#pragma unroll
        for (int i = 0; i < IPW_A; ++i) {
          const int ga = wave * IPW_A + i;
          const int hi = hi0[i] + s_kh, wi = wi0[i] + s_kw;
          const bool ok = mok[i] & kvalid & ((unsigned)hi < (unsigned)a.H) & ((unsigned)wi < (unsigned)a.W);
          const bf16_t* src = xg + (xbase[i] + koff + chunk8[ga & 1]);
          src = ok ? src : zp;
          dma16(src, sbase + ga * 1024);
        }
      } else {
#pragma unroll
        for (int i = 0; i < IPW_A; ++i) {
          const int ga = wave * IPW_A + i;
          const int par = ga & 1;
          const int hi = hi0[i] + kkh[par], wi = wi0[i] + kkw[par];
          const bool ok = mok[i] & (kkh[par] < a.KH) & ((unsigned)hi < (unsigned)a.H) & ((unsigned)wi < (unsigned)a.W);
          const bf16_t* src = xg + (xbase[i] + (kkh[par] * a.W + kkw[par]) * a.x_cs + kc[par]);
          src = ok ? src : zp;
          dma16(src, sbase + ga * 1024);
        }
      }
#pragma unroll
      for (int i = 0; i < IPW_B; ++i) {
        const int gb = wave * IPW_B + i;
        const bf16_t* src = wsrc[i] + (size_t)gi_kt * BKE;
        src = nok[i] ? src : zp;
        dma16(src, sbase + BM * 128 + gb * 1024);
      }
      if constexpr (ALIGNED) {
        s_c0 += BKE;
        if (s_c0 >= a.Cin) {
          s_c0 = 0;
          if (++s_kw == a.KW) {
            s_kw = 0;
            ++s_kh;
          }
        }
      } else {
#pragma unroll
        for (int par = 0; par < 2; ++par) {
          kc[par] += BKE;
          while (kc[par] >= a.Cin) {
            kc[par] -= a.Cin;
            if (++kkw[par] == a.KW) {
              kkw[par] = 0;
              ++kkh[par];
            }
          }
        }
      }
      ++gi;
      if (++gi_kt == nk) {
        gi_kt = 0;
        ++gi_r;
      }
    };
#pragma unroll
    for (int p = 0; p < AHEAD; ++p)
      if (gi < total) issue();
    for (int g = 0; g < total; ++g) {
      const int pending = min(AHEAD - 1, total - 1 - g);
      if (pending >= 2)
        wait_vmcnt<2 * LPT>();
      else if (pending == 1)
        wait_vmcnt<LPT>();
      else
        wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();
      if (gi < total) issue();
    }
    return;
  }

  // ---- MFMA waves ---------------------------------------------------------------------------------------------------------
  const int fr = lane & 15, fg = lane >> 4;
  const uint32_t sw = (fr >> 1) & 7;
  const uint32_t x_off0 = (wm * (BM / WM) + fr) * 128 + (((0 + fg) ^ sw) & 7) * 16;
  const uint32_t x_off1 = (wm * (BM / WM) + fr) * 128 + (((4 + fg) ^ sw) & 7) * 16;
  const uint32_t w_off0 = (BM + wn * (BN / WN) + fr) * 128 + (((0 + fg) ^ sw) & 7) * 16;
  const uint32_t w_off1 = (BM + wn * (BN / WN) + fr) * 128 + (((4 + fg) ^ sw) & 7) * 16;
  int mrow[TM];
#pragma unroll
  for (int j = 0; j < TM; ++j) {
    const int m = bm0 + wm * (BM / WM) + j * 16 + (lane & 15);
    mrow[j] = m < a.M ? m : -1;
  }
  int g = 0;
  for (int r = r_begin; r < r_end; ++r) {
    f32x4_t acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nk; ++kt, ++g) {
      __builtin_amdgcn_s_barrier();
      const uint32_t sb = lds0 + (g % NSTAGE) * STAGE_BYTES;
      u32x4_t xf0[TM], xf1[TM], wf0[TN], wf1[TN];
      static_assert(TM + TN <= 15, "lgkmcnt holds 4 bits");
      static_for<0, TN>([&](auto i) { wf0[i] = lds_read128<decltype(i)::value * 2048>(sb + w_off0); });
      static_for<0, TM>([&](auto j) { xf0[j] = lds_read128<decltype(j)::value * 2048>(sb + x_off0); });
      static_for<0, TN>([&](auto i) { wf1[i] = lds_read128<decltype(i)::value * 2048>(sb + w_off1); });
      static_for<0, TM>([&](auto j) { xf1[j] = lds_read128<decltype(j)::value * 2048>(sb + x_off1); });
      asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(TM + TN) : "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j)
          acc[i][j] = Half16<HT>::mfma(__builtin_bit_cast(bf16x8_t, wf0[i]),
                                                              __builtin_bit_cast(bf16x8_t, xf0[j]), acc[i][j]);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j)
          acc[i][j] = Half16<HT>::mfma(__builtin_bit_cast(bf16x8_t, wf1[i]),
                                                              __builtin_bit_cast(bf16x8_t, xf1[j]), acc[i][j]);
    }
    int p = 0;
    for (int i = 1; i < n_members; ++i)
      if (r >= args[i].blk0) p = i;
    conv_store_tiles<HT, TN, TM>(args[p], acc, (r - args[p].blk0) * BN + wn * (BN / WN), (lane >> 4) * 4, mrow);
  }
}

template <typename HT, int BM, int BN, int WM, int WN, int NSTAGE>
__global__ __launch_bounds__(dma_threads(WM, WN, NSTAGE)) void conv_igemm_dma_walk_kernel(const ConvArgs* __restrict__ args, int n, int total,
                                                                                         int split) {
  // split 2 ("paired walk"): the walk of a pixel tile is shared by two workgroups with consecutive logical ids -- they start
  // together on ONE XCD, stream the pixel rows at the same time (one fetch from the memory side for both) and re-read them
  // from an L2 that holds 16 pixel tiles per XCD instead of 32 (K = 768: 196 KB each)
  const int l = xcd_tile_index(total);
  if (l < 0) return;
  const int bm = l / split, part = l - bm * split;
  const int R = args[0].grp_nt;                  // out-channel tiles of all members
  const int r0 = R * part / split, r1 = R * (part + 1) / split;
  if (r0 >= r1) return;
  if (args[0].Cin % 64 == 0)
    conv_igemm_dma_walk_body<HT, BM, BN, WM, WN, NSTAGE, true>(args, n, bm, r0, r1);
  else
    conv_igemm_dma_walk_body<HT, BM, BN, WM, WN, NSTAGE, false>(args, n, bm, r0, r1);
}

template <typename HT, int BM, int BN, int WM, int WN, int NSTAGE, bool ALIGNED>
__global__ __launch_bounds__(dma_threads(WM, WN, NSTAGE)) void conv_igemm_dma_kernel(ConvArgs a) {
  const int tiles_n = (a.Cout + BN - 1) / BN;
  int bm, bn;
  if (a.remap) {
    const int l = xcd_tile_index(a.tiles_m * tiles_n);
    if (l < 0) return;
    bn = l % tiles_n;
    bm = l / tiles_n;
  } else {
    if ((int)blockIdx.x >= a.tiles_m * tiles_n) return;
    bm = blockIdx.x % a.tiles_m;
    bn = blockIdx.x / a.tiles_m;
  }
  conv_igemm_dma_body<HT, BM, BN, WM, WN, NSTAGE, ALIGNED>(a, bm, bn);
}

// Grouped launch: blockIdx.z selects one of several independent convolutions (the same-depth
// ops of the parallel Inception branches) whose argument records live in device memory.  One
// launch then carries 2-4x the workgroups of a single 12x12 / 5x5 layer, which is what those
// layers lack to fill 256 CUs at batch 64.
template <typename HT, int BM, int BN, int WM, int WN, int NSTAGE>
__global__ __launch_bounds__(dma_threads(WM, WN, NSTAGE)) void conv_igemm_dma_grouped_kernel(const ConvArgs* __restrict__ args, int n, int total) {
  int bid = blockIdx.x;
  const int remap = args[0].remap;
  if (remap) {
    bid = xcd_tile_index(total);
    if (bid < 0) return;
  } else if (bid >= total) {
    return;
  }
  if (remap == 2) {
    // shared input: logical id = (pixel tile, out-channel tile over ALL members), pixel tile slowest, and every
    // XCD owns a contiguous range of logical ids -- the members' workgroups of one pixel tile run together on one
    // XCD, so the activation rows come from the memory side once instead of once per member
    const int R = args[0].grp_nt;
    const int bm = bid / R, r = bid - bm * R;
    int p = 0;
    for (int i = 1; i < n; ++i)
      if (r >= args[i].blk0) p = i;
    const ConvArgs a = args[p];
    if (a.Cin % 64 == 0)
      conv_igemm_dma_body<HT, BM, BN, WM, WN, NSTAGE, true>(a, bm, r - a.blk0);
    else
      conv_igemm_dma_body<HT, BM, BN, WM, WN, NSTAGE, false>(a, bm, r - a.blk0);
    return;
  }
  int p = 0;
  for (int i = 1; i < n; ++i)
    if (bid >= args[i].blk0) p = i;
  const ConvArgs a = args[p];
  const int local = bid - a.blk0;
  if (a.member_kind == 1) {
    pool_bn_relu_member<HT>(a, local);
    return;
  }
  int bm, bn;
  if (remap) {
    const int tiles_n = (a.Cout + BN - 1) / BN;
    bn = local % tiles_n;
    bm = local / tiles_n;
  } else {
    // the out-channel tiles of a pixel tile 8 workgroups apart: consecutive workgroup ids go round the 8 XCDs, so b and
    // b + 8 start together on ONE XCD and the second reads the im2col rows the first has just pulled into that L2
    // (3x3 / 2 288 -> 384 of Mixed_6a at 1280 images: 2.5 GB of reads per launch, every tap of either tile from the memory side)
    // The pairing is between `local` and `local + 8`, i.e. hardware ids bid and bid + 8 (this branch runs without the
    // xcd_tile_index remap: bid == blockIdx.x), which share an XCD whatever a.blk0 is -- a member need not start on a
    // multiple of 8; only WHICH XCD a pair lands on moves with blk0.
    const int tiles_n = (a.Cout + BN - 1) / BN;
    const int full = a.tiles_m & ~7;
    if (local < full * tiles_n) {
      bn = (local >> 3) % tiles_n;
      bm = (local / (8 * tiles_n)) * 8 + (local & 7);
    } else {
      const int l2 = local - full * tiles_n, r = a.tiles_m - full;
      bm = full + l2 % r;
      bn = l2 / r;
    }
  }
  if (a.Cin % 64 == 0)
    conv_igemm_dma_body<HT, BM, BN, WM, WN, NSTAGE, true>(a, bm, bn);
  else
    conv_igemm_dma_body<HT, BM, BN, WM, WN, NSTAGE, false>(a, bm, bn);
}

// comic_cnn_op::min_lds: lower bound on the dynamic LDS a DMA conv workgroup requests.  84 KiB admits one
// workgroup per CU instead of 2-3: a forward that runs on a second stream UNDER the decoder step then leaves
// wave slots, registers and LDS for the latency-bound decoder kernels (measured: forward alone 1.44 -> 1.79 ms,
// overlapped training step 3.67 -> 3.53 ms).  Carried per op (ConvArgs::min_lds), no process state.

#include "conv_patch.inc"

template <typename HT, int BM, int BN, int WM, int WN, int NSTAGE>
int launch_dma_grouped(const ConvArgs* args_dev, int n, int total_blocks, int min_lds, hipStream_t st) {
  constexpr int lds0 = ring_stages(NSTAGE) * (BM + BN) * 128;
  const int lds = std::max(lds0, min_lds);
  static PerDeviceOnce attr_once__;
  bool& attr_set = attr_once__.slot();   // hipFuncSetAttribute holds per device
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)conv_igemm_dma_grouped_kernel<HT, BM, BN, WM, WN, NSTAGE>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
      comic_set_error("conv: cannot reserve %d bytes of LDS", lds);
      return 1;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL((conv_igemm_dma_grouped_kernel<HT, BM, BN, WM, WN, NSTAGE>), dim3((total_blocks + 7) / 8 * 8),
                     dim3(dma_threads(WM, WN, NSTAGE)), lds, st, args_dev, n, total_blocks);
  return 0;
}

template <typename HT, int BM, int BN, int WM, int WN, int NSTAGE>
int launch_dma_walk(const ConvArgs* args_dev, int n, int total_blocks, int min_lds, hipStream_t st, int split = 1) {
  constexpr int lds0 = ring_stages(NSTAGE) * (BM + BN) * 128;
  const int lds = std::max(lds0, min_lds);
  static PerDeviceOnce attr_once__;
  bool& attr_set = attr_once__.slot();
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)conv_igemm_dma_walk_kernel<HT, BM, BN, WM, WN, NSTAGE>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
      comic_set_error("conv: cannot reserve %d bytes of LDS", lds);
      return 1;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL((conv_igemm_dma_walk_kernel<HT, BM, BN, WM, WN, NSTAGE>), dim3((total_blocks + 7) / 8 * 8),
                     dim3(dma_threads(WM, WN, NSTAGE)), lds, st, args_dev, n, total_blocks, split);
  return 0;
}

template <typename HT, int BM, int BN, int WM, int WN, int NSTAGE = 3>
int launch_dma(const ConvArgs& a, hipStream_t st) {
  static_assert(ring_stages(NSTAGE) >= 2 && ring_stages(NSTAGE) <= 4, "pipeline depth");
  constexpr int lds0 = ring_stages(NSTAGE) * (BM + BN) * 128;
  const int lds = std::max(lds0, a.min_lds);
  static_assert(lds0 <= 160 * 1024, "LDS");
  static PerDeviceOnce attr_once__;
  bool& attr_set = attr_once__.slot();   // hipFuncSetAttribute holds per device
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)conv_igemm_dma_kernel<HT, BM, BN, WM, WN, NSTAGE, true>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void*)conv_igemm_dma_kernel<HT, BM, BN, WM, WN, NSTAGE, false>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
      comic_set_error("conv: cannot reserve %d bytes of LDS", lds);
      return 1;
    }
    attr_set = true;
  }
  ConvArgs b = a;
  b.tiles_m = cdiv(a.M, BM);
  const long total = (long)b.tiles_m * cdiv(a.Cout, BN);
  if (total >= (1L << 31) - 8) {
    comic_set_error("conv: too many tiles");
    return 1;
  }
  dim3 grid((unsigned)((total + 7) / 8 * 8));
  if (a.Cin % 64 == 0)
    hipLaunchKernelGGL((conv_igemm_dma_kernel<HT, BM, BN, WM, WN, NSTAGE, true>), grid, dim3(dma_threads(WM, WN, NSTAGE)), lds, st, b);
  else
    hipLaunchKernelGGL((conv_igemm_dma_kernel<HT, BM, BN, WM, WN, NSTAGE, false>), grid, dim3(dma_threads(WM, WN, NSTAGE)), lds, st, b);
  return 0;
}

// Backward-data launches fused with the producer's activation gradient (ConvArgs::mask_y): the im2col kernel with the MASK
// epilogue, the tile shapes the backward of small batches uses.
template <int BM, int BN, int WM, int WN, int NSTAGE, bool ALIGNED>
__global__ __launch_bounds__(dma_threads(WM, WN, NSTAGE)) void conv_igemm_dma_mask_kernel(ConvArgs a) {
  const int tiles_n = (a.Cout + BN - 1) / BN;
  const int l = xcd_tile_index(a.tiles_m * tiles_n);
  if (l < 0) return;
  conv_igemm_dma_body<bf16_t, BM, BN, WM, WN, NSTAGE, ALIGNED, true>(a, l / tiles_n, l % tiles_n);
}

template <int BM, int BN, int WM, int WN, int NSTAGE = 3>
int launch_dma_mask(const ConvArgs& a, hipStream_t st) {
  constexpr int lds0 = ring_stages(NSTAGE) * (BM + BN) * 128;
  const int lds = std::max(lds0, a.min_lds);
  static PerDeviceOnce attr_once__;
  bool& attr_set = attr_once__.slot();
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)conv_igemm_dma_mask_kernel<BM, BN, WM, WN, NSTAGE, true>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void*)conv_igemm_dma_mask_kernel<BM, BN, WM, WN, NSTAGE, false>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
      comic_set_error("conv: cannot reserve %d bytes of LDS", lds);
      return 1;
    }
    attr_set = true;
  }
  ConvArgs b = a;
  b.remap = 1;
  b.tiles_m = cdiv(a.M, BM);
  const long total = (long)b.tiles_m * cdiv(a.Cout, BN);
  if (total >= (1L << 31) - 8) {
    comic_set_error("conv: too many tiles");
    return 1;
  }
  dim3 grid((unsigned)((total + 7) / 8 * 8));
  if (a.Cin % 64 == 0)
    hipLaunchKernelGGL((conv_igemm_dma_mask_kernel<BM, BN, WM, WN, NSTAGE, true>), grid, dim3(dma_threads(WM, WN, NSTAGE)), lds, st, b);
  else
    hipLaunchKernelGGL((conv_igemm_dma_mask_kernel<BM, BN, WM, WN, NSTAGE, false>), grid, dim3(dma_threads(WM, WN, NSTAGE)), lds, st, b);
  return 0;
}

int dispatch_igemm_dma_mask(const ConvArgs& a, hipStream_t st) {
  const long b128x128 = (long)cdiv(a.M, 128) * cdiv(a.Cout, 128);
  const long b128x64 = (long)cdiv(a.M, 128) * cdiv(a.Cout, 64);
  const long b64x64 = (long)cdiv(a.M, 64) * cdiv(a.Cout, 64);
  if (a.Cout <= 32) return launch_dma_mask<128, 32, 4, 1>(a, st);
  if (a.Cout % 128 == 0 && b128x128 >= 512) return launch_dma_mask<128, 128, 2, 2>(a, st);
  if (b128x64 >= 512) return launch_dma_mask<128, 64, 2, 2>(a, st);
  if (b64x64 >= 384) return launch_dma_mask<64, 64, 2, 2>(a, st);
  return launch_dma_mask<32, 64, 1, 4>(a, st);
}

// Image-resident kernel (conv_img.hip): n convs of ONE shape (same source geometry, Cin, Cout) as one launch.
int img_config(const ConvArgs& a) {
  if (!a.w_frag || a.accum || a.mask_y || a.x_cs % 8 != 0 || a.x_co % 8 != 0) return -1;
  return comic_img_config(a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.SH, a.SW, a.Ho, a.Wo);
}
bool img_same_shape(const ConvArgs& p, const ConvArgs& q) {
  return p.H == q.H && p.W == q.W && p.Cin == q.Cin && p.Cout == q.Cout && p.B == q.B;
}
template <typename HT>
int launch_img_convs(const ConvArgs* a, int n, hipStream_t st) {
  const int cfg = img_config(a[0]);
  if (cfg < 0 || n < 1 || n > kImgMaxMembers) {
    comic_set_error("conv: layer not eligible for the image-resident kernel (%dx%d, %dx%d, Cin %d, Cout %d%s)", a[0].H, a[0].W,
                    a[0].KH, a[0].KW, a[0].Cin, a[0].Cout, a[0].w_frag ? "" : ", no fragment-order weights");
    return 3;
  }
  ComicImgArgs ia;
  memset(&ia, 0, sizeof(ia));
  ia.n_members = n;
  ia.f16 = std::is_same<HT, f16_t>::value;
  ia.B = a[0].B; ia.H = a[0].H; ia.W = a[0].W; ia.Cin = a[0].Cin; ia.Cout = a[0].Cout;
  ia.G = comic_img_images_per_group(cfg);
  ia.groups = cdiv(ia.B, ia.G);
  const int pxb = a[0].Cin * 2;
  ia.PXBp = pxb + ((pxb % 64 == 0) ? 32 : 0);
  ia.KS32 = a[0].Kpad / 32;
  for (int j = 0; j < n; ++j) {
    if (img_config(a[j]) != cfg || !img_same_shape(a[j], a[0])) {
      comic_set_error("conv: the members of an image-resident launch must have one shape");
      return 3;
    }
    ComicImgMember& m = ia.m[j];
    m.x = (const bf16_t*)a[j].x; m.wf = (const bf16_t*)a[j].w_frag; m.scale = a[j].scale; m.shift = a[j].shift; m.y = a[j].y;
    m.x_cs = a[j].x_cs; m.x_co = a[j].x_co; m.y_cs = a[j].y_cs; m.y_co = a[j].y_co;
    m.KH = a[j].KH; m.KW = a[j].KW; m.PT = a[j].PT; m.PL = a[j].PL; m.relu = a[j].relu; m.out_f32 = a[j].out_f32;
  }
  return comic_img_launch(cfg, ia, st);
}

int validate_grouped_conv(const comic_cnn_op* op, int xc, int yc, const comic_conv_weight* wt, int batch);
// Chains of image-resident convs (COMIC_CHAIN_TILE, conv_img.hip conv_img_chain_kernel): the n ops of the group are one or
// two chains, chain after chain; an op with COMIC_OP_CHAIN_LINK hands its output to the NEXT op of the table through the LDS
// (its dst buffer is not written), an op without it ends its chain and stores to its dst slice.
template <typename HT>
int launch_img_chains(const comic_cnn_op* op, int n, void* const* buffers, const int32_t* buf_channels,
                      const comic_conv_weight* weights, int batch, hipStream_t st) {
  ComicChainArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.f16 = std::is_same<HT, f16_t>::value;
  ca.B = batch; ca.H = op[0].H; ca.W = op[0].W; ca.Cin = op[0].Cin;
  const int pxb = ca.Cin * 2;
  ca.PXBp = pxb + ((pxb % 64 == 0) ? 32 : 0);
  COMIC_REQUIRE(comic_img_chain_supported(ca.H, ca.W, ca.Cin), "conv chain: %dx%d maps of %d channels are not supported", ca.H,
                ca.W, ca.Cin);
  int nm = 0;
  for (int j = 0; j < n;) {
    COMIC_REQUIRE(nm < kChainMaxMembers, "conv chain: more than %d chains in one launch", kChainMaxMembers);
    ComicChainMember& m = ca.m[nm];
    int len = 0;
    for (;; ++len) {
      COMIC_REQUIRE(j + len < n && len < kChainMaxConvs, "conv chain: a chain of more than %d convs, or a link flag on the last op",
                    kChainMaxConvs);
      const comic_cnn_op* o = op + j + len;
      const comic_conv_weight* wt = weights + o->weight;
      const bool link = (o->flags & COMIC_OP_CHAIN_LINK) != 0;
      if (int rc = validate_grouped_conv(o, buf_channels[o->src], buf_channels[o->dst], wt, batch)) return rc;
      COMIC_REQUIRE(o->SH == 1 && o->SW == 1 && o->Ho == o->H && o->Wo == o->W && o->H == ca.H && o->W == ca.W &&
                        o->Cin == ca.Cin && o->KH * o->KW >= 2 && o->KH * o->KW <= 32 && !(o->flags & (COMIC_OP_RAW | COMIC_OP_X3)),
                    "conv chain: every conv must be a stride-1 SAME conv with BatchNorm over the chain's %dx%dx%d input", ca.H, ca.W,
                    ca.Cin);
      COMIC_REQUIRE(wt->w_frag, "conv chain: no fragment-order weights");
      COMIC_REQUIRE(o->Cout == (link ? ca.Cin : 192), "conv chain: inner convs keep the channel count, the last one has 192 outputs");
      COMIC_REQUIRE(!link || (!o->out_f32 && o->dst == o[1].src && o->dst_coff == 0 && o[1].src_coff == 0 &&
                              buf_channels[o->dst] == ca.Cin),
                    "conv chain: a linked conv must feed the next op of the table");
      ComicChainConv& c = m.c[len];
      c.wf = (const bf16_t*)wt->w_frag; c.scale = wt->scale; c.shift = wt->shift;
      c.KH = o->KH; c.KW = o->KW; c.PT = o->PT; c.PL = o->PL; c.Cout = o->Cout; c.relu = o->relu;
      c.KS32 = ((o->KH * o->KW * o->Cin + 63) / 64 * 64) / 32;
      c.keep = nullptr;
      if (link && (o->flags & COMIC_OP_CHAIN_KEEP)) {
        COMIC_REQUIRE(buffers[o->dst] && buf_channels[o->dst] % 4 == 0, "conv chain: a kept intermediate map needs its buffer");
        c.keep = buffers[o->dst]; c.keep_cs = buf_channels[o->dst]; c.keep_co = o->dst_coff;
      }
      if (len == 0) {
        COMIC_REQUIRE(buf_channels[o->src] % 8 == 0 && o->src_coff % 8 == 0 && buffers[o->src], "conv chain: bad source slice");
        m.x = (const bf16_t*)buffers[o->src]; m.x_cs = buf_channels[o->src]; m.x_co = o->src_coff;
      }
      if (!link) {
        COMIC_REQUIRE(buffers[o->dst], "conv chain: null destination");
        m.y = buffers[o->dst]; m.y_cs = buf_channels[o->dst]; m.y_co = o->dst_coff; m.out_f32 = o->out_f32;
        ++len;
        break;
      }
    }
    m.n_convs = len;
    j += len;
    ++nm;
  }
  if (nm == 2 && ca.m[1].n_convs > ca.m[0].n_convs) std::swap(ca.m[0], ca.m[1]);     // the longer chain's workgroups first
  ca.n_members = nm;
  return comic_img_chain_launch(ca, st);
}

// explicit tile selection (comic_cnn_op.tile, filled by the host-side autotuner)
constexpr int kNumConvTiles = 12;
// ids 26..28: two-stage wide im2col tiles.  The L2 -> LDS fill (about 30 B/clk/CU) bounds the im2col kernel: a k-tile
// costs (BM+BN)*128 bytes of fill for BM*BN/32 MFMA cycles, so 64x128 cannot pass ~31 % of the MFMA peak, 128x128
// 47 %, 128x192 56 %; with two stages (instead of three) two such workgroups still share a CU.
constexpr int kWideTile0 = 26, kNumWideTiles = 22;      // 35..47: four MFMA waves + four loader waves      // 29..31: 8 waves, one workgroup per CU (fill bound 62 / 80 / 94 %)
// 56..58: "walk" forms of 44 / 38 / 35 for launches whose members share their im2col matrix (conv_igemm_dma_walk_body)
constexpr int kWalkTile0 = 56, kNumWalkTiles = 6;      // 56..58: one workgroup per pixel tile; 59..61: two (paired walk)
inline int walk_split(int t) { return t >= kWalkTile0 + 3 ? 2 : 1; }
inline bool is_walk_tile(int t) { return t >= kWalkTile0 && t < kWalkTile0 + kNumWalkTiles; }
inline bool is_im2col_tile(int t) { return t <= kNumConvTiles || (t >= kWideTile0 && t < kWideTile0 + kNumWideTiles) || is_walk_tile(t); }
template <typename HT>
int launch_dma_tile(int tile, const ConvArgs& a, hipStream_t st) {
  switch (tile) {
    case 26: return launch_dma<HT, 128, 128, 2, 2, 2>(a, st);
    case 27: return launch_dma<HT, 128, 192, 2, 2, 2>(a, st);
    case 28: return launch_dma<HT, 192, 128, 2, 2, 2>(a, st);
    case 29: return launch_dma<HT, 256, 128, 4, 2, 2>(a, st);
    case 30: return launch_dma<HT, 256, 192, 2, 4, 2>(a, st);
    case 31: return launch_dma<HT, 256, 256, 2, 4, 2>(a, st);
    case 32: return launch_dma<HT, 128, 160, 2, 2, 2>(a, st);      // 160-channel layers without a ragged column tile
    case 33: return launch_dma<HT, 256, 64, 4, 1, 2>(a, st);
    case 34: return launch_dma<HT, 192, 96, 2, 2, 2>(a, st);
    case 35: return launch_dma<HT, 128, 192, 2, 2, kLoaderWaves + 3>(a, st);
    case 36: return launch_dma<HT, 128, 128, 2, 2, kLoaderWaves + 3>(a, st);
    case 37: return launch_dma<HT, 128, 256, 2, 2, kLoaderWaves + 3>(a, st);
    case 38: return launch_dma<HT, 192, 128, 2, 2, kLoaderWaves + 3>(a, st);
    case 39: return launch_dma<HT, 128, 160, 2, 2, kLoaderWaves + 3>(a, st);
    case 40: return launch_dma<HT, 192, 192, 2, 2, kLoaderWaves + 2>(a, st);
    case 41: return launch_dma<HT, 128, 192, 2, 2, kLoaderWaves + 4>(a, st);
    case 42: return launch_dma<HT, 160, 192, 2, 2, kLoaderWaves + 3>(a, st);
    case 43: return launch_dma<HT, 192, 160, 2, 2, kLoaderWaves + 3>(a, st);
    case 44: return launch_dma<HT, 192, 192, 2, 2, kLoaderWaves + 3>(a, st);
    case 45: return launch_dma<HT, 64, 128, 2, 2, kLoaderWaves + 3>(a, st);        // small-batch shapes
    case 46: return launch_dma<HT, 128, 64, 2, 2, kLoaderWaves + 3>(a, st);
    case 47: return launch_dma<HT, 64, 64, 2, 2, kLoaderWaves + 4>(a, st);
    case 1: return launch_dma<HT, 128, 128, 2, 2, 3>(a, st);
    case 2: return launch_dma<HT, 128, 64, 2, 2, 3>(a, st);
    case 3: return launch_dma<HT, 64, 64, 2, 2, 3>(a, st);
    case 4: return launch_dma<HT, 32, 64, 1, 4, 3>(a, st);
    case 5: return launch_dma<HT, 128, 32, 4, 1, 3>(a, st);
    case 6: return launch_dma<HT, 64, 128, 2, 2, 3>(a, st);
    case 7: return launch_dma<HT, 256, 64, 4, 1, 3>(a, st);
    case 8: return launch_dma<HT, 128, 64, 2, 2, 4>(a, st);
    case 9: return launch_dma<HT, 64, 64, 2, 2, 4>(a, st);
    case 10: return launch_dma<HT, 32, 64, 1, 4, 4>(a, st);
    case 11: return launch_dma<HT, 64, 128, 2, 2, 4>(a, st);
    case 12: return launch_dma<HT, 128, 32, 4, 1, 4>(a, st);
    // patch-resident variants (stride 1, Cin >= 32): 64*TM pixels x 16*TN channels
    case 13: return launch_patch<HT, 4, 4>(a, st);
    case 14: return launch_patch<HT, 4, 2>(a, st);
    case 15: return launch_patch<HT, 4, 6>(a, st);
    case 16: return launch_patch<HT, 2, 4>(a, st);
    case 17: return launch_patch<HT, 2, 2>(a, st);
    case 18: return launch_patch<HT, 2, 6>(a, st);
    // patch-resident, 8 / 12 waves per workgroup (2-3 per SIMD) over one patch
    case 19: return launch_patch<HT, 4, 4, 4, 2>(a, st);    // 256 px x 128 ch
    case 20: return launch_patch<HT, 4, 4, 4, 3>(a, st);    // 256 px x 192 ch
    case 21: return launch_patch<HT, 4, 4, 8, 1>(a, st);    // 512 px x 64 ch
    case 22: return launch_patch<HT, 4, 2, 4, 2>(a, st);    // 256 px x 64 ch, 8 waves
    case 23: return launch_patch<HT, 4, 6, 4, 2>(a, st);    // 256 px x 192 ch, 8 waves
    case 24: return launch_patch<HT, 2, 4, 4, 2>(a, st);    // 128 px x 128 ch
    case 25: return launch_patch<HT, 2, 6, 4, 2>(a, st);    // 128 px x 192 ch, 8 waves
    // patch-resident, four MFMA waves + four loader waves
    case 48: return launch_patch<HT, 4, 4, 4, 1, kLoaderWaves + 3>(a, st);   // 256 px x 64 ch
    case 49: return launch_patch<HT, 4, 2, 4, 1, kLoaderWaves + 3>(a, st);   // 256 px x 32 ch
    case 50: return launch_patch<HT, 4, 6, 4, 1, kLoaderWaves + 3>(a, st);   // 256 px x 96 ch
    case 51: return launch_patch<HT, 2, 6, 4, 1, kLoaderWaves + 3>(a, st);   // 128 px x 96 ch
    case 52: return launch_patch<HT, 4, 6, 2, 2, kLoaderWaves + 3>(a, st);   // 128 px x 192 ch
    case 53: return launch_patch<HT, 4, 4, 2, 2, kLoaderWaves + 3>(a, st);   // 128 px x 128 ch
    case COMIC_IMG_TILE: return launch_img_convs<HT>(&a, 1, st);             // image-resident (conv_img.hip)
    default:
      comic_set_error("conv: unknown tile id %d", tile);
      return 2;
  }
}

// (BM, BN) of the explicit tile ids above
constexpr int kTileBM[kNumConvTiles + 1] = {0, 128, 128, 64, 32, 128, 64, 256, 128, 64, 32, 64, 128};
constexpr int kTileBN[kNumConvTiles + 1] = {0, 128, 64, 64, 64, 32, 128, 64, 64, 64, 64, 128, 32};
constexpr int kWideBM[kNumWideTiles] = {128, 128, 192, 256, 256, 256, 128, 256, 192, 128, 128, 128, 192, 128, 192, 128, 160, 192, 192, 64, 128, 64};
constexpr int kWideBN[kNumWideTiles] = {128, 192, 128, 128, 192, 256, 160, 64, 96, 192, 128, 256, 128, 160, 192, 192, 192, 160, 192, 128, 64, 64};
constexpr int kWalkBase[kNumWalkTiles] = {44, 38, 35, 44, 38, 35};
inline int im2col_tile_threads(int t) { return (t >= 29 && t <= 31) || t >= 35 ? 512 : 256; }
inline int tile_bm(int t) { return is_walk_tile(t) ? kWideBM[kWalkBase[t - kWalkTile0] - kWideTile0] : t >= kWideTile0 ? kWideBM[t - kWideTile0] : kTileBM[t]; }
inline int tile_bn(int t) { return is_walk_tile(t) ? kWideBN[kWalkBase[t - kWalkTile0] - kWideTile0] : t >= kWideTile0 ? kWideBN[t - kWideTile0] : kTileBN[t]; }

template <typename HT>
int launch_dma_grouped_tile(int tile, const ConvArgs* args_dev, int n, int total_blocks, int min_lds, hipStream_t st) {
  switch (tile) {
    case 26: return launch_dma_grouped<HT, 128, 128, 2, 2, 2>(args_dev, n, total_blocks, min_lds, st);
    case 27: return launch_dma_grouped<HT, 128, 192, 2, 2, 2>(args_dev, n, total_blocks, min_lds, st);
    case 28: return launch_dma_grouped<HT, 192, 128, 2, 2, 2>(args_dev, n, total_blocks, min_lds, st);
    case 29: return launch_dma_grouped<HT, 256, 128, 4, 2, 2>(args_dev, n, total_blocks, min_lds, st);
    case 30: return launch_dma_grouped<HT, 256, 192, 2, 4, 2>(args_dev, n, total_blocks, min_lds, st);
    case 31: return launch_dma_grouped<HT, 256, 256, 2, 4, 2>(args_dev, n, total_blocks, min_lds, st);
    case 32: return launch_dma_grouped<HT, 128, 160, 2, 2, 2>(args_dev, n, total_blocks, min_lds, st);
    case 33: return launch_dma_grouped<HT, 256, 64, 4, 1, 2>(args_dev, n, total_blocks, min_lds, st);
    case 34: return launch_dma_grouped<HT, 192, 96, 2, 2, 2>(args_dev, n, total_blocks, min_lds, st);
    case 35: return launch_dma_grouped<HT, 128, 192, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, min_lds, st);
    case 36: return launch_dma_grouped<HT, 128, 128, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, min_lds, st);
    case 37: return launch_dma_grouped<HT, 128, 256, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, min_lds, st);
    case 38: return launch_dma_grouped<HT, 192, 128, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, min_lds, st);
    case 39: return launch_dma_grouped<HT, 128, 160, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, min_lds, st);
    case 40: return launch_dma_grouped<HT, 192, 192, 2, 2, kLoaderWaves + 2>(args_dev, n, total_blocks, min_lds, st);
    case 41: return launch_dma_grouped<HT, 128, 192, 2, 2, kLoaderWaves + 4>(args_dev, n, total_blocks, min_lds, st);
    case 42: return launch_dma_grouped<HT, 160, 192, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, min_lds, st);
    case 43: return launch_dma_grouped<HT, 192, 160, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, min_lds, st);
    case 44: return launch_dma_grouped<HT, 192, 192, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, min_lds, st);
    case 45: return launch_dma_grouped<HT, 64, 128, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, min_lds, st);
    case 46: return launch_dma_grouped<HT, 128, 64, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, min_lds, st);
    case 47: return launch_dma_grouped<HT, 64, 64, 2, 2, kLoaderWaves + 4>(args_dev, n, total_blocks, min_lds, st);
    case 56: return launch_dma_walk<HT, 192, 192, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, min_lds, st);
    case 57: return launch_dma_walk<HT, 192, 128, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, min_lds, st);
    case 58: return launch_dma_walk<HT, 128, 192, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, min_lds, st);
    case 59: return launch_dma_walk<HT, 192, 192, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, min_lds, st, 2);
    case 60: return launch_dma_walk<HT, 192, 128, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, min_lds, st, 2);
    case 61: return launch_dma_walk<HT, 128, 192, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, min_lds, st, 2);
    case 1: return launch_dma_grouped<HT, 128, 128, 2, 2, 3>(args_dev, n, total_blocks, min_lds, st);
    case 2: return launch_dma_grouped<HT, 128, 64, 2, 2, 3>(args_dev, n, total_blocks, min_lds, st);
    case 3: return launch_dma_grouped<HT, 64, 64, 2, 2, 3>(args_dev, n, total_blocks, min_lds, st);
    case 4: return launch_dma_grouped<HT, 32, 64, 1, 4, 3>(args_dev, n, total_blocks, min_lds, st);
    case 5: return launch_dma_grouped<HT, 128, 32, 4, 1, 3>(args_dev, n, total_blocks, min_lds, st);
    case 6: return launch_dma_grouped<HT, 64, 128, 2, 2, 3>(args_dev, n, total_blocks, min_lds, st);
    case 7: return launch_dma_grouped<HT, 256, 64, 4, 1, 3>(args_dev, n, total_blocks, min_lds, st);
    case 8: return launch_dma_grouped<HT, 128, 64, 2, 2, 4>(args_dev, n, total_blocks, min_lds, st);
    case 9: return launch_dma_grouped<HT, 64, 64, 2, 2, 4>(args_dev, n, total_blocks, min_lds, st);
    case 10: return launch_dma_grouped<HT, 32, 64, 1, 4, 4>(args_dev, n, total_blocks, min_lds, st);
    case 11: return launch_dma_grouped<HT, 64, 128, 2, 2, 4>(args_dev, n, total_blocks, min_lds, st);
    case 12: return launch_dma_grouped<HT, 128, 32, 4, 1, 4>(args_dev, n, total_blocks, min_lds, st);
    default:
      comic_set_error("conv: unknown tile id %d", tile);
      return 2;
  }
}

// Tile of a group: the explicit id of its first member, else the same fill rule as the
// single-conv heuristic applied to the group's total tile count.

// ---- weight-stationary 1x1 groups (conv_ws.hip) ---------------------------------------------------------------
// ops[0..n) qualify when they are 1x1 / stride-1 / unpadded convolutions over the SAME source slice (the convs at
// the head of an Inception block, or a single conv), Cin and the concatenated Cout fit the register-resident
// weight layout, and -- with COMIC_OP_POOLED_SRC -- every member reads through the same 3x3 / 2 VALID max-pool.
bool ws_group_eligible(const comic_cnn_op* ops, int n) {
  if (n < 1 || n > 4) return false;
  int tiles = 0;
  for (int j = 0; j < n; ++j) {
    const comic_cnn_op& o = ops[j];
    if (o.kind != 0 || o.KH != 1 || o.KW != 1 || o.SH != 1 || o.SW != 1 || o.PT != 0 || o.PL != 0) return false;
    if (o.src != ops[0].src || o.src_coff != ops[0].src_coff || o.Cin != ops[0].Cin || o.H != ops[0].H ||
        o.W != ops[0].W || o.Ho != ops[0].Ho || o.Wo != ops[0].Wo || (o.flags & COMIC_OP_POOLED_SRC) != (ops[0].flags & COMIC_OP_POOLED_SRC))
      return false;
    if (o.Cout % 16 != 0 || (o.flags & COMIC_OP_X3)) return false;   // (conv_ws.hip has its own epilogue: plain stores)
    tiles += o.Cout / 16;
  }
  const comic_cnn_op& o = ops[0];
  if (o.flags & COMIC_OP_POOLED_SRC) {
    if (o.Ho != (o.H - 3) / 2 + 1 || o.Wo != (o.W - 3) / 2 + 1) return false;
  } else if (o.Ho != o.H || o.Wo != o.W) {
    return false;
  }
  return comic_ws_supported(o.Cin, tiles);
}

template <typename HT>
int run_ws_group(const comic_cnn_op* ops, int n, void* const* buffers, const int32_t* buf_channels,
                 const comic_conv_weight* weights, int batch, hipStream_t st) {
  COMIC_REQUIRE(ws_group_eligible(ops, n), "conv_ws: ops are not an eligible 1x1 group (kind %d, %dx%d, Cin %d)", ops[0].kind,
                ops[0].KH, ops[0].KW, ops[0].Cin);
  ComicWsArgs a;
  memset(&a, 0, sizeof(a));
  const comic_cnn_op& o = ops[0];
  const int xc = buf_channels[o.src];
  COMIC_REQUIRE(buffers[o.src] && o.src_coff + o.Cin <= xc && xc % 8 == 0 && o.src_coff % 8 == 0, "conv_ws: bad source slice");
  COMIC_REQUIRE((long)batch * o.H * o.W * xc * 2 < (1L << 31), "conv_ws: activation tensor too large");
  a.x = (const bf16_t*)buffers[o.src];
  a.B = batch; a.H = o.H; a.W = o.W; a.x_cs = xc; a.x_co = o.src_coff; a.Cin = o.Cin;
  a.Kpad = (o.Cin + 63) / 64 * 64;
  a.Ho = o.Ho; a.Wo = o.Wo; a.M = batch * o.Ho * o.Wo;
  a.pooled = (o.flags & COMIC_OP_POOLED_SRC) ? 1 : 0;
  a.n_members = n;
  a.f16 = std::is_same<HT, f16_t>::value;
  a.tiles_m = cdiv(a.M, 64);
  int t0 = 0;
  for (int j = 0; j < n; ++j) {
    const comic_cnn_op& q = ops[j];
    const comic_conv_weight* wt = weights + q.weight;
    const bool raw = (q.flags & COMIC_OP_RAW) != 0;
    const int yc = buf_channels[q.dst];
    COMIC_REQUIRE(wt->w && (raw || (wt->scale && wt->shift)), "conv_ws: missing weights");
    COMIC_REQUIRE(buffers[q.dst] && q.dst_coff + q.Cout <= yc && q.dst_coff % 4 == 0 && yc % 4 == 0, "conv_ws: bad destination slice");
    COMIC_REQUIRE((long)a.M * yc < (1L << 31), "conv_ws: output tensor too large");
    ComicWsMember& m = a.m[j];
    m.w = (const bf16_t*)wt->w;
    m.scale = raw ? nullptr : wt->scale;
    m.shift = raw ? nullptr : wt->shift;
    m.y = buffers[q.dst];
    m.y_cs = yc; m.y_co = q.dst_coff; m.cout = q.Cout; m.relu = q.relu; m.out_f32 = q.out_f32;
    m.tile0 = t0;
    t0 += q.Cout / 16;
  }
  a.n_tiles = t0;
  if (int rc = comic_ws_launch(a, st)) return rc;
  COMIC_LAUNCH_CHECK("conv_ws");
  return 0;
}
// WS is the default (tile id 0) for an eligible group with enough pixel tiles to occupy every CU
bool ws_group_selected(const comic_cnn_op* ops, int n, int batch) {
  if (!ws_group_eligible(ops, n)) return false;
  if (ops[0].flags & COMIC_OP_POOLED_SRC) return true;
  if (ops[0].tile == COMIC_WS_TILE) return true;
  return ops[0].tile == 0 && (long)batch * ops[0].Ho * ops[0].Wo >= 64L * 256;
}

int group_tile(const comic_cnn_op* ops, int n, int batch) {
  if (ops[0].tile == COMIC_IMG_TILE || ops[0].tile == COMIC_CHAIN_TILE) return ops[0].tile;
  if (ops[0].tile > 0 && ops[0].tile < COMIC_WS_TILE) return ops[0].tile;
  if (is_walk_tile(ops[0].tile)) return ops[0].tile;
  bool all128 = true;
  for (int i = 0; i < n; ++i) all128 = all128 && ops[i].Cout % 128 == 0;
  auto blocks = [&](int t) {
    long b = 0;
    for (int i = 0; i < n; ++i)
      b += (long)cdiv(batch * ops[i].Ho * ops[i].Wo, kTileBM[t]) * cdiv(ops[i].Cout, kTileBN[t]);
    return b;
  };
  if (all128 && blocks(1) >= 512) return 1;
  if (blocks(2) >= 512) return 2;
  if (blocks(3) >= 384) return 3;
  return 4;
}

// Workgroup layout of one group member under tile id `tile`: sets a.tiles_m (and the patch geometry for the
// patch-resident ids), returns its workgroup count or -1 when the member is not eligible; *lds = LDS it needs.
long member_blocks(int tile, ConvArgs& a, int* lds) {
  if (a.member_kind == 1) {          // pool + BN + ReLU items, kPoolItemsPerThread per thread of the launch's workgroup size
    const int threads = is_im2col_tile(tile) ? im2col_tile_threads(tile) : kPatchTiles[patch_tile_index(tile)].threads;
    *lds = 0;
    return cdiv64((long)a.M * (a.Cin / 4), (long)threads * kPoolItemsPerThread);
  }
  if (is_im2col_tile(tile)) {
    a.tiles_m = cdiv(a.M, tile_bm(tile));
    *lds = 0;
    return (long)a.tiles_m * cdiv(a.Cout, tile_bn(tile));
  }
  const PatchTile pt = kPatchTiles[patch_tile_index(tile)];
  PatchGeo g;
  if (!patch_geometry(a, pt.BM, pt.BN, 3, g)) return -1;
  apply_geometry(a, g);
  *lds = g.lds_bytes;
  return (long)a.tiles_m * cdiv(a.Cout, pt.BN);
}

template <typename HT>
int dispatch_igemm_dma(const ConvArgs& a, hipStream_t st) {
  // thin-channel stride-1 layers with many pixels (the 109x109 / 52x52 / 25x25 3x3 and 5x5 convs, forward and
  // backward-data): the patch-resident kernel, variants as the autotuner picks them at batch 64
  if (a.SH == 1 && a.SW == 1 && a.Cin >= 32 && a.Cin <= 96 && a.KH * a.KW > 1 && a.M >= 16384) {
    PatchGeo g;
    if (a.Cout <= 32 && patch_geometry(a, 256, 32, 3, g)) return launch_patch<HT, 4, 2>(a, st);
    if (a.Cout == 96 && patch_geometry(a, 128, 96, 3, g)) return launch_patch<HT, 2, 6>(a, st);
    if (patch_geometry(a, 256, 64, 3, g)) return launch_patch<HT, 4, 2, 4, 2>(a, st);
  }
  const long b128x128 = (long)cdiv(a.M, 128) * cdiv(a.Cout, 128);
  const long b128x64 = (long)cdiv(a.M, 128) * cdiv(a.Cout, 64);
  const long b64x64 = (long)cdiv(a.M, 64) * cdiv(a.Cout, 64);
  if (a.Cout <= 32) return launch_dma<HT, 128, 32, 4, 1>(a, st);
  if (a.Cout % 128 == 0 && b128x128 >= 512) return launch_dma<HT, 128, 128, 2, 2>(a, st);
  if (b128x64 >= 512) return launch_dma<HT, 128, 64, 2, 2>(a, st);
  if (b64x64 >= 384) return launch_dma<HT, 64, 64, 2, 2>(a, st);
  return launch_dma<HT, 32, 64, 1, 4>(a, st);
}

const void* zero_page_address() {
  static const void* p[16] = {nullptr};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  if (!p[dev]) {
    void* q = nullptr;
    if (hipGetSymbolAddress(&q, HIP_SYMBOL(g_zero_page)) == hipSuccess) p[dev] = q;
  }
  return p[dev];
}

template <typename T, int BM, int BN, int WM, int WN>
void launch_igemm(const ConvArgs& a, hipStream_t st) {
  dim3 grid(cdiv(a.M, BM), cdiv(a.Cout, BN));
  hipLaunchKernelGGL((conv_igemm_kernel<T, BM, BN, WM, WN>), grid, dim3(256), 0, st, a);
}

template <typename T>
void launch_igemm_mask(const ConvArgs& a, hipStream_t st) {     // fused activation gradient (backward of the fp32 plan)
  dim3 grid(cdiv(a.M, 64), cdiv(a.Cout, 64));
  hipLaunchKernelGGL((conv_igemm_kernel<T, 64, 64, 2, 2, true>), grid, dim3(256), 0, st, a);
}

template <typename T>
int dispatch_igemm(const ConvArgs& a, hipStream_t st) {
  // choose the largest tile that still gives >= ~2 workgroups per CU; small layers fall
  // back to 64x64 (XCD note: grid.x = pixel tiles, so workgroups b, b+8 share an L2 and a
  // neighbouring input window).
  const int n64 = cdiv(a.Cout, 64);
  const long blocks_128x128 = (long)cdiv(a.M, 128) * cdiv(a.Cout, 128);
  const long blocks_128x64 = (long)cdiv(a.M, 128) * n64;
  if (a.Cout <= 32) {
    launch_igemm<T, 128, 32, 4, 1>(a, st);
  } else if (a.Cout % 128 == 0 && blocks_128x128 >= 512) {
    launch_igemm<T, 128, 128, 2, 2>(a, st);
  } else if (blocks_128x64 >= 512) {
    launch_igemm<T, 128, 64, 2, 2>(a, st);
  } else {
    launch_igemm<T, 64, 64, 2, 2>(a, st);
  }
  return 0;
}

int fill_args(ConvArgs& a, const comic_cnn_op* op, const void* x, int x_channels, void* y, int y_channels,
              const comic_conv_weight* wt, int batch) {
  a.x = x;
  a.y = y;
  a.w = wt ? wt->w : nullptr;
  const bool raw = op->kind == 0 && (op->flags & COMIC_OP_RAW);     // epilogue deferred to a kind-7 op
  a.scale = (wt && !raw) ? wt->scale : nullptr;
  a.shift = (wt && !raw) ? wt->shift : nullptr;
  a.B = batch;
  a.H = op->H; a.W = op->W; a.Cin = op->Cin; a.Cout = op->Cout;
  a.KH = op->KH; a.KW = op->KW; a.SH = op->SH; a.SW = op->SW; a.PT = op->PT; a.PL = op->PL;
  a.Ho = op->Ho; a.Wo = op->Wo;
  a.x_cs = x_channels; a.x_co = op->src_coff; a.y_cs = y_channels; a.y_co = op->dst_coff;
  a.K = op->KH * op->KW * op->Cin;
  a.Kpad = (a.K + 63) / 64 * 64;
  a.M = batch * op->Ho * op->Wo;
  a.relu = op->relu;
  a.out_f32 = op->out_f32;
  a.zero = zero_page_address();
  a.blk0 = 0;
  a.tiles_m = 0;
  a.accum = 0;
  a.mask_y = nullptr;
  a.mask_scale = nullptr;
  a.mask_dbeta = nullptr;
  a.mask_cs = a.mask_co = 0;
  a.member_kind = 0;
  a.w_frag = wt ? wt->w_frag : nullptr;
  a.min_lds = std::min(std::max(op->min_lds, 0), 160 * 1024);
  a.remap = 1;
  // COMIC_OP_X3: bf16 buffers hold [hi | lo | hi] regions of a third of their channels each
  const bool x3 = (op->flags & COMIC_OP_X3) != 0;
  a.x3 = (x3 && !op->out_f32) ? y_channels / 3 : 0;
  a.x3_src = (x3 && op->kind >= 2 && op->kind <= 3) ? x_channels / 3 : 0;
  return 0;
}

}  // namespace

// the per-op launcher (declared in conv_run.h: the backward's backward-data launches come through here too)
template <typename T>
int comic_run_op(const comic_cnn_op* op, const void* x, int xc, void* y, int yc, const comic_conv_weight* wt, int batch,
                 hipStream_t st, int accum, const ConvMask* mask) {
  constexpr int EPC = Elem<T>::EPC;
  ConvArgs a;
  fill_args(a, op, x, xc, y, yc, wt, batch);
  a.accum = accum;
  if (mask) {
    COMIC_REQUIRE(op->kind == 0 && !accum && !op->out_f32 && !a.x3 && !a.scale, "conv: fused activation gradient on a plain backward-data launch only");
    a.mask_y = mask->y;
    a.mask_cs = mask->y_cs;
    a.mask_co = mask->y_co;
    a.mask_scale = mask->scale;
    a.mask_dbeta = mask->dbeta;
  }
  COMIC_REQUIRE(x && y, "cnn op %d: null buffer", op->kind);
  COMIC_REQUIRE((long)batch * op->H * op->W * xc < (1L << 31) && (long)a.M * yc < (1L << 31),
                "cnn op: tensor exceeds 2^31 elements");
  COMIC_REQUIRE(op->src_coff + op->Cin <= xc, "cnn op: source channel slice out of range");
  switch (op->kind) {
    case 0: {
      COMIC_REQUIRE(wt && wt->w && (accum || mask || (op->flags & COMIC_OP_RAW) || (wt->scale && wt->shift)), "conv: missing weights");
      COMIC_REQUIRE(op->Cin % EPC == 0 && op->src_coff % EPC == 0 && xc % EPC == 0,
                    "conv: Cin/offset/stride must be multiples of %d", EPC);
      COMIC_REQUIRE(op->Cout % 16 == 0 && op->dst_coff % 4 == 0 && yc % 4 == 0,
                    "conv: Cout must be a multiple of 16 (got %d)", op->Cout);
      COMIC_REQUIRE(op->dst_coff + op->Cout <= (a.x3 ? a.x3 : yc), "conv: destination channel slice out of range");
      COMIC_REQUIRE(!(op->flags & COMIC_OP_X3) || (std::is_same<T, bf16_t>::value && yc % 3 == 0 && (yc / 3) % 4 == 0 && !accum),
                    "conv: COMIC_OP_X3 needs a bf16 plan and a destination of three equal channel regions");
      if constexpr (sizeof(T) == 2) {
        COMIC_REQUIRE(a.zero, "conv: zero page symbol not resolvable");
        COMIC_REQUIRE((long)batch * op->H * op->W * xc * 2 < (1L << 31), "conv: activation tensor too large");
        if (mask) {
          COMIC_REQUIRE((std::is_same<T, bf16_t>::value), "conv: the fused activation gradient is a bf16-plan launch");
          if (int rc = dispatch_igemm_dma_mask(a, st)) return rc;
        } else if (op->tile > 0) {
          if (int rc = launch_dma_tile<T>(op->tile, a, st)) return rc;
        } else if (int rc = dispatch_igemm_dma<T>(a, st)) {
          return rc;
        }
      } else if (mask) {
        launch_igemm_mask<T>(a, st);
      } else {
        dispatch_igemm<T>(a, st);
      }
      break;
    }
    case 1: {
      COMIC_REQUIRE(wt && wt->w, "stem conv: missing weights");
      COMIC_REQUIRE(op->Cin <= 4 && op->Cout % 32 == 0, "stem conv: needs Cin<=4, Cout%%32==0");
      COMIC_REQUIRE(op->dst_coff % 4 == 0 && yc % 4 == 0, "stem conv: misaligned destination");
      const size_t lds = (size_t)a.K * a.Cout * sizeof(float);
      COMIC_REQUIRE(lds <= 64 * 1024, "stem conv: weights do not fit LDS");
      if (a.K <= 32 && a.Cout == 32 && a.PT == 0 && a.PL == 0 && (op->Ho - 1) * op->SH + op->KH <= op->H &&
          (op->Wo - 1) * op->SW + op->KW <= op->W && op->tile != 1)
        hipLaunchKernelGGL((conv_stem_mfma_kernel<T, 2>), dim3(cdiv(a.M, 1024)), dim3(256), 0, st, a);   // VALID 3x3x3
      else if (const int lrow = ((op->PL + op->W + op->KW) * op->Cin + kStemKRow + 1) / 2 * 2;   // staged row, floats
               sizeof(T) == 2 && op->tile != 1 && a.Cout == 64 && op->KW * op->Cin <= kStemKRow && op->KH <= 8 &&
               xc == op->Cin && op->src_coff == 0 && (op->W * op->Cin) % 2 == 0 && (op->PL * op->Cin) % 2 == 0 &&
               (op->SW * op->Cin) % 2 == 0 && kStemRows * op->Wo <= 256 &&
               (op->Wo - 1) * op->SW * op->Cin + kStemKRow <= lrow &&          // the last pixel's widest operand read
               ((kStemRows - 1) * op->SH + op->KH) * (op->W * op->Cin / 2) <= kStemFetch * 256 &&
               2 * lrow * ((kStemRows - 1) * op->SH + 8) * 4 <= 64 * 1024) {
        // Inception-V1 Conv2d_1a_7x7 (7x7 / 2, SAME) -- conv_stem_wide_kernel, persistent workgroups (one per CU: the
        // filter fragments take most of the register file)
        const int bpi = cdiv(op->Ho, kStemRows), total = batch * bpi;
        const int lds_w = 2 * lrow * ((kStemRows - 1) * op->SH + 8) * 4;
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        hipLaunchKernelGGL((conv_stem_wide_kernel<typename Half16Of<T>::type, 4, 6>), dim3(std::min(total, cus)), dim3(256), lds_w, st, a, lrow, bpi, total);
      }
      else
        hipLaunchKernelGGL((conv_stem_kernel<T>), dim3(cdiv(a.M, 256)), dim3(256), lds, st, a);
      break;
    }
    case 2:
    case 3: {
      COMIC_REQUIRE(op->Cin % EPC == 0 && op->src_coff % EPC == 0 && xc % EPC == 0 && op->dst_coff % EPC == 0 &&
                        yc % EPC == 0,
                    "pool: channel counts/offsets must be multiples of %d", EPC);
      COMIC_REQUIRE(op->dst_coff + op->Cin <= yc, "pool: destination channel slice out of range");
      const long total = (long)a.M * (op->Cin / EPC);
      if (op->flags & COMIC_OP_X3) {
        if constexpr (std::is_same<T, bf16_t>::value) {
          COMIC_REQUIRE(xc % 3 == 0 && yc % 3 == 0 && a.x3 > 0 && a.x3_src > 0 && op->src_coff + op->Cin <= a.x3_src &&
                            op->dst_coff + op->Cin <= a.x3 && a.x3 % 8 == 0 && a.x3_src % 8 == 0,
                        "pool (x3): channel regions do not fit the buffers");
          if (op->kind == 2)
            hipLaunchKernelGGL((pool_x3_kernel<0>), dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, a);
          else
            hipLaunchKernelGGL((pool_x3_kernel<1>), dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, a);
          break;
        } else {
          COMIC_REQUIRE(false, "pool: COMIC_OP_X3 is a bf16-plan layout");
        }
      }
      // row-walking form when there are enough rows to occupy the chip (op->tile: 1 forces it, 2 forces the per-pixel form)
      if (op->kind == 2 && op->KH == 3 && op->KW == 3 && op->SH == 1 && op->SW == 1 && op->PT == 1 && op->PL == 1 &&
          op->Ho == op->H && op->Wo == op->W &&
          (op->tile == 1 || (op->tile == 0 && (long)batch * op->H * (op->Cin / EPC) >= 256L * 256)))
        hipLaunchKernelGGL((maxpool3_rows_kernel<T>), dim3((unsigned)cdiv64((long)batch * op->H * (op->Cin / EPC), 256)), dim3(256),
                           0, st, a);
      else if (op->kind == 2)
        hipLaunchKernelGGL((pool_kernel<T, 0>), dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, a);
      else
        hipLaunchKernelGGL((pool_kernel<T, 1>), dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, a);
      break;
    }
    case 4: {
      COMIC_REQUIRE(op->Cin % EPC == 0 && op->src_coff % EPC == 0 && xc % EPC == 0, "global pool: misaligned");
      COMIC_REQUIRE((op->Ho - 1) * op->SH + op->KH <= op->H && (op->Wo - 1) * op->SW + op->KW <= op->W,
                    "global pool: window exceeds input (VALID only)");
      const long total = (long)a.M * (op->Cin / EPC);
      hipLaunchKernelGGL((global_avgpool_kernel<T>), dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, a);
      break;
    }
    case 7: {
      COMIC_REQUIRE(wt && wt->scale && wt->shift, "pool+bn: missing scale / shift");
      COMIC_REQUIRE(op->KH == 3 && op->KW == 3 && op->SH == 1 && op->SW == 1 && op->PT == 1 && op->PL == 1 &&
                        op->Ho == op->H && op->Wo == op->W && op->Cin == op->Cout,
                    "pool+bn: 3x3 stride-1 SAME only");
      COMIC_REQUIRE(op->Cin % 4 == 0 && op->src_coff % 4 == 0 && xc % 4 == 0 && op->dst_coff % 4 == 0 && yc % 4 == 0,
                    "pool+bn: channel counts/offsets must be multiples of 4");
      COMIC_REQUIRE(op->dst_coff + op->Cin <= (a.x3 ? a.x3 : yc), "pool+bn: destination channel slice out of range");
      const long total = (long)a.M * (op->Cin / 4);
      a.out_f32 = (op->out_f32 || sizeof(T) == 4) ? 1 : 0;
      // row-walking form when there are enough rows to occupy the chip (op->tile: 1 forces it, 2 forces the per-pixel form)
      if (op->tile == 1 || (op->tile == 0 && (long)batch * op->H * (op->Cin / 4) >= 256L * 256))
        hipLaunchKernelGGL(pool_bn_relu_rows_kernel<typename Half16Of<T>::type>, dim3((unsigned)cdiv64((long)batch * op->H * (op->Cin / 4), 256)), dim3(256),
                           0, st, a);
      else
        hipLaunchKernelGGL(pool_bn_relu_kernel<typename Half16Of<T>::type>, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, a);
      break;
    }
    default:
      COMIC_REQUIRE(false, "unknown cnn op kind %d", op->kind);
  }
  COMIC_LAUNCH_CHECK("cnn op");
  return 0;
}
template int comic_run_op<float>(const comic_cnn_op*, const void*, int, void*, int, const comic_conv_weight*, int, hipStream_t, int, const ConvMask*);
template int comic_run_op<bf16_t>(const comic_cnn_op*, const void*, int, void*, int, const comic_conv_weight*, int, hipStream_t, int, const ConvMask*);
template int comic_run_op<f16_t>(const comic_cnn_op*, const void*, int, void*, int, const comic_conv_weight*, int, hipStream_t, int, const ConvMask*);

namespace {

int validate_grouped_conv(const comic_cnn_op* op, int xc, int yc, const comic_conv_weight* wt, int batch) {
  if (op->kind == 7) {               // pool + BN + ReLU member (same checks as the stand-alone launch)
    COMIC_REQUIRE(wt && wt->scale && wt->shift, "pool+bn: missing scale / shift");
    COMIC_REQUIRE(op->KH == 3 && op->KW == 3 && op->SH == 1 && op->SW == 1 && op->PT == 1 && op->PL == 1 &&
                      op->Ho == op->H && op->Wo == op->W && op->Cin == op->Cout && op->src_f32,
                  "pool+bn: 3x3 stride-1 SAME over an fp32 source only");
    COMIC_REQUIRE(op->Cin % 4 == 0 && op->src_coff % 4 == 0 && xc % 4 == 0 && op->dst_coff % 4 == 0 && yc % 4 == 0,
                  "pool+bn: channel counts/offsets must be multiples of 4");
    COMIC_REQUIRE(op->src_coff + op->Cin <= xc && op->dst_coff + op->Cin <= yc, "pool+bn: channel slice out of range");
    COMIC_REQUIRE((long)batch * op->H * op->W * xc < (1L << 31) && (long)batch * op->Ho * op->Wo * yc < (1L << 31),
                  "pool+bn: tensor too large");
    return 0;
  }
  COMIC_REQUIRE(op->kind == 0, "grouped launch: op kind %d is not a conv", op->kind);
  COMIC_REQUIRE(wt && wt->w && wt->scale && wt->shift, "conv: missing weights");
  COMIC_REQUIRE(op->Cin % 8 == 0 && op->src_coff % 8 == 0 && xc % 8 == 0, "conv: Cin/offset/stride must be multiples of 8");
  COMIC_REQUIRE(op->Cout % 16 == 0 && op->dst_coff % 4 == 0 && yc % 4 == 0, "conv: Cout must be a multiple of 16 (got %d)",
                op->Cout);
  COMIC_REQUIRE(op->src_coff + op->Cin <= xc, "conv: source channel slice out of range");
  COMIC_REQUIRE(op->dst_coff + op->Cout <= yc, "conv: destination channel slice out of range");
  COMIC_REQUIRE((long)batch * op->H * op->W * xc * 2 < (1L << 31) && (long)batch * op->Ho * op->Wo * yc < (1L << 31),
                "conv: activation tensor too large");
  return 0;
}

// All members of a grouped launch are convolutions over the SAME im2col matrix (same source slice, filter window,
// stride and padding -- the 1x1 convs at the head of an Inception block): the launch may then order its
// workgroups by pixel tile (ConvArgs::remap == 2).
bool shared_input_group(const ConvArgs* a, int n) {
  if (n < 2) return false;
  for (int j = 0; j < n; ++j) {
    if (a[j].member_kind != 0) return false;
    if (a[j].x != a[0].x || a[j].x_co != a[0].x_co || a[j].x_cs != a[0].x_cs || a[j].Cin != a[0].Cin ||
        a[j].KH != a[0].KH || a[j].KW != a[0].KW || a[j].SH != a[0].SH || a[j].SW != a[0].SW || a[j].PT != a[0].PT ||
        a[j].PL != a[0].PL || a[j].M != a[0].M || a[j].tiles_m != a[0].tiles_m)
      return false;
  }
  return true;
}

// length of the group run starting at ops[i] (1 when ungrouped)
int group_run(const comic_cnn_op* ops, int n_ops, int i) {
  if (ops[i].group <= 0) return 1;
  int j = i + 1;
  while (j < n_ops && ops[j].group == ops[i].group) ++j;
  return j - i;
}

}  // namespace

extern "C" long comic_cnn_group_args_bytes(const comic_cnn_op* ops, int n_ops) {
  long n = 0;
  for (int i = 0; i < n_ops; ++i) n += ops[i].group > 0;
  return n * (long)sizeof(ConvArgs);
}

extern "C" int comic_cnn_build_group_args(const comic_cnn_op* ops, int n_ops, void* const* buffers,
                                          const int32_t* buf_channels, const comic_conv_weight* weights, int batch,
                                          void* host_out) {
  COMIC_REQUIRE(ops && buffers && buf_channels && weights && host_out, "comic_cnn_build_group_args: null argument");
  ConvArgs* out = (ConvArgs*)host_out;
  for (int i = 0; i < n_ops;) {
    const int n = group_run(ops, n_ops, i);
    if (ops[i].group <= 0) {
      ++i;
      continue;
    }
    if (ws_group_selected(ops + i, n, batch)) {       // conv_ws.hip takes its arguments by value
      memset(out, 0, sizeof(ConvArgs) * n);
      out += n;
      i += n;
      continue;
    }
    COMIC_REQUIRE(ops[i].tile != COMIC_WS_TILE, "conv: group is not eligible for the weight-stationary 1x1 kernel");
    const int tile = group_tile(ops + i, n, batch);
    for (int j = 0; j < n; ++j)
      COMIC_REQUIRE(tile == COMIC_CHAIN_TILE || !(ops[i + j].flags & COMIC_OP_CHAIN_LINK),
                    "conv: COMIC_OP_CHAIN_LINK ops depend on each other -- their group runs on COMIC_CHAIN_TILE only (got tile %d)", tile);
    if (tile == COMIC_IMG_TILE || tile == COMIC_CHAIN_TILE) {      // conv_img.hip takes its arguments by value, too
      memset(out, 0, sizeof(ConvArgs) * n);
      out += n;
      i += n;
      continue;
    }
    int blk = 0;
    for (int j = 0; j < n; ++j) {
      const comic_cnn_op* op = ops + i + j;
      const comic_conv_weight* wt = weights + op->weight;
      if (int rc = validate_grouped_conv(op, buf_channels[op->src], buf_channels[op->dst], wt, batch)) return rc;
      COMIC_REQUIRE(buffers[op->src] && buffers[op->dst], "grouped conv: null buffer");
      ConvArgs& a = out[j];
      fill_args(a, op, buffers[op->src], buf_channels[op->src], buffers[op->dst], buf_channels[op->dst], wt, batch);
      COMIC_REQUIRE(a.zero, "conv: zero page symbol not resolvable");
      a.member_kind = op->kind == 7 ? 1 : 0;
      a.blk0 = blk;
      a.remap = 0;   // members differ in K: contiguous per-XCD ranges would put the heavy ones on few XCDs
      int lds = 0;
      const long nb = member_blocks(tile, a, &lds);
      COMIC_REQUIRE(nb >= 0, "grouped conv: member %d (stride %d, Cin %d) is not eligible for patch tile %d", j, op->SH,
                    op->Cin, tile);
      blk += (int)nb;
    }
    COMIC_REQUIRE(!is_walk_tile(tile) || shared_input_group(out, n),
                  "conv: tile %d walks over members that share their im2col matrix; this launch's do not", tile);
    if (is_im2col_tile(tile) && shared_input_group(out, n)) {
      int nt = 0;
      for (int j = 0; j < n; ++j) {
        out[j].remap = is_walk_tile(tile) ? 3 : 2;     // 3: one workgroup per pixel tile walks all nt out-channel tiles
        out[j].blk0 = nt;
        nt += cdiv(out[j].Cout, tile_bn(tile));
      }
      for (int j = 0; j < n; ++j) out[j].grp_nt = nt;
    }
    out += n;
    i += n;
  }
  return 0;
}

extern "C" int comic_conv2d_bn_relu(const comic_cnn_op* op, const void* x, int x_channels, void* y, int y_channels,
                                    const comic_conv_weight* wt, int batch, int dtype, void* stream) {
  COMIC_REQUIRE(op, "null op");
  hipStream_t st = (hipStream_t)stream;
  const bool half = dtype == COMIC_BF16 || dtype == COMIC_F16;   // the 16-bit plans
  if (op->kind == 0 && half &&
      ((op->flags & COMIC_OP_POOLED_SRC) || op->tile == COMIC_WS_TILE || (op->tile == 0 && ws_group_selected(op, 1, batch)))) {
    // a single 1x1 conv on the weight-stationary kernel (conv_ws.hip): one-member group over a two-entry buffer table
    comic_cnn_op o = *op;
    o.src = 0; o.dst = 1; o.weight = 0;
    void* const bufs[2] = {(void*)x, y};
    const int32_t chans[2] = {x_channels, y_channels};
    COMIC_REQUIRE(wt, "conv: missing weights");
    if (dtype == COMIC_F16) return run_ws_group<f16_t>(&o, 1, bufs, chans, wt, batch, st);
    return run_ws_group<bf16_t>(&o, 1, bufs, chans, wt, batch, st);
  }
  COMIC_REQUIRE(!(op->kind == 0 && (op->flags & COMIC_OP_POOLED_SRC)), "conv: COMIC_OP_POOLED_SRC needs a bf16 or f16 plan");
  if (half && op->src_f32) {
    COMIC_REQUIRE(op->kind == 4 || op->kind == 7, "src_f32 is only supported by the global average pool and pool+bn");
    if (op->kind == 7 && dtype == COMIC_F16) return comic_run_op<f16_t>(op, x, x_channels, y, y_channels, wt, batch, st);
    if (op->kind == 7) return comic_run_op<bf16_t>(op, x, x_channels, y, y_channels, wt, batch, st);
    return comic_run_op<float>(op, x, x_channels, y, y_channels, wt, batch, st);
  }
  if (dtype == COMIC_BF16) return comic_run_op<bf16_t>(op, x, x_channels, y, y_channels, wt, batch, st);
  if (dtype == COMIC_F16) return comic_run_op<f16_t>(op, x, x_channels, y, y_channels, wt, batch, st);
  if (dtype == COMIC_F32) return comic_run_op<float>(op, x, x_channels, y, y_channels, wt, batch, st);
  COMIC_REQUIRE(false, "unknown dtype %d", dtype);
  return 2;
}

namespace {
// Branch lanes: three internal non-blocking streams + fork/join events per device, created on
// first use and kept for the life of the process (the only objects this library owns).
struct Lanes {
  hipStream_t s[3];
  hipEvent_t fork_ev, join_ev[3];
  bool ok = false;
};
Lanes* get_lanes() {
  static Lanes lanes[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  Lanes& l = lanes[dev];
  if (!l.ok) {
    for (int i = 0; i < 3; ++i) {
      if (hipStreamCreateWithFlags(&l.s[i], hipStreamNonBlocking) != hipSuccess) return nullptr;
      if (hipEventCreateWithFlags(&l.join_ev[i], hipEventDisableTiming) != hipSuccess) return nullptr;
    }
    if (hipEventCreateWithFlags(&l.fork_ev, hipEventDisableTiming) != hipSuccess) return nullptr;
    l.ok = true;
  }
  return &l;
}
}  // namespace

// HT: the 16-bit format of the grouped launches and the stem stream (bf16_t for the fp32 plans, which have neither)
template <typename HT>
static int cnn_forward_impl(const comic_cnn_op* ops, int n_ops, void* const* buffers, const int32_t* buf_channels,
                            const comic_conv_weight* weights, int batch, int dtype, const void* group_args_dev,
                            void* stream) {
  COMIC_REQUIRE(ops && buffers && buf_channels, "comic_cnn_forward: null table");
  const ConvArgs* gargs = (const ConvArgs*)group_args_dev;
  hipStream_t main_st = (hipStream_t)stream;
  Lanes* lanes = nullptr;
  bool used[3] = {false, false, false};
  for (int i = 0; i < n_ops; ++i) {
    const comic_cnn_op* op = ops + i;
    if (op->kind == 5) {  // fork
      if (!lanes) lanes = get_lanes();
      COMIC_REQUIRE(lanes, "comic_cnn_forward: cannot create branch streams");
      COMIC_REQUIRE(hipEventRecord(lanes->fork_ev, main_st) == hipSuccess, "fork: event record failed");
      for (int l = 0; l < 3; ++l) {
        COMIC_REQUIRE(hipStreamWaitEvent(lanes->s[l], lanes->fork_ev, 0) == hipSuccess, "fork: wait failed");
        used[l] = false;
      }
      continue;
    }
    if (op->kind == 6) {  // join
      COMIC_REQUIRE(lanes, "join without fork");
      for (int l = 0; l < 3; ++l) {
        if (!used[l]) continue;
        COMIC_REQUIRE(hipEventRecord(lanes->join_ev[l], lanes->s[l]) == hipSuccess, "join: event record failed");
        COMIC_REQUIRE(hipStreamWaitEvent(main_st, lanes->join_ev[l], 0) == hipSuccess, "join: wait failed");
      }
      continue;
    }
    if (gargs && op->group > 0) {
      COMIC_REQUIRE(dtype == Half16<HT>::code && (op->kind == 0 || op->kind == 7) && op->lane == 0,
                    "grouped launch needs a bf16 or f16 plan and conv / pool+bn ops on the caller's stream");
      const int n = group_run(ops, n_ops, i);
      if (ws_group_selected(op, n, batch)) {
        if (int rc = run_ws_group<HT>(op, n, buffers, buf_channels, weights, batch, main_st)) return rc;
        gargs += n;
        i += n - 1;
        continue;
      }
      COMIC_REQUIRE(op->tile != COMIC_WS_TILE, "conv: group is not eligible for the weight-stationary 1x1 kernel");
      const int tile = group_tile(op, n, batch);
      for (int j = 0; j < n; ++j)
        COMIC_REQUIRE(tile == COMIC_CHAIN_TILE || !(op[j].flags & COMIC_OP_CHAIN_LINK),
                      "conv: COMIC_OP_CHAIN_LINK ops depend on each other -- their group runs on COMIC_CHAIN_TILE only (got tile %d)", tile);
      if (tile == COMIC_CHAIN_TILE) {
        if (int rc = launch_img_chains<HT>(op, n, buffers, buf_channels, weights, batch, main_st)) return rc;
        COMIC_LAUNCH_CHECK("image-resident conv chains");
        gargs += n;
        i += n - 1;
        continue;
      }
      if (tile == COMIC_IMG_TILE) {
        // members of one shape share a launch; a member of another shape (7x1 128 -> 192 beside 1x7 128 -> 128) gets its own
        COMIC_REQUIRE(n <= kImgMaxMembers, "grouped launch: too many members for the image-resident kernel");
        ConvArgs ma[kImgMaxMembers];
        bool done[kImgMaxMembers] = {false, false, false, false};
        for (int j = 0; j < n; ++j) {
          COMIC_REQUIRE(op[j].kind == 0, "grouped launch: the image-resident kernel takes convolutions only");
          if (int rc = validate_grouped_conv(op + j, buf_channels[op[j].src], buf_channels[op[j].dst], weights + op[j].weight, batch)) return rc;
          fill_args(ma[j], op + j, buffers[op[j].src], buf_channels[op[j].src], buffers[op[j].dst], buf_channels[op[j].dst],
                    weights + op[j].weight, batch);
        }
        for (int j = 0; j < n; ++j) {
          if (done[j]) continue;
          ConvArgs run[kImgMaxMembers];
          int nr = 0;
          for (int q = j; q < n; ++q)
            if (!done[q] && img_same_shape(ma[q], ma[j])) {
              run[nr++] = ma[q];
              done[q] = true;
            }
          if (int rc = launch_img_convs<HT>(run, nr, main_st)) return rc;
        }
        COMIC_LAUNCH_CHECK("image-resident conv group");
        gargs += n;
        i += n - 1;
        continue;
      }
      long blocks = 0;
      int lds_max = 0;
      for (int j = 0; j < n; ++j) {
        ConvArgs a;
        fill_args(a, op + j, buffers[op[j].src], buf_channels[op[j].src], buffers[op[j].dst], buf_channels[op[j].dst],
                  weights + op[j].weight, batch);
        a.member_kind = op[j].kind == 7 ? 1 : 0;
        int lds = 0;
        const long nb = member_blocks(tile, a, &lds);
        COMIC_REQUIRE(nb >= 0, "grouped launch: member %d is not eligible for patch tile %d", j, tile);
        blocks += nb;
        lds_max = std::max(lds_max, lds);
      }
      COMIC_REQUIRE(blocks > 0 && blocks < (1L << 31), "grouped launch: bad workgroup count");
      if (is_walk_tile(tile)) blocks = (long)cdiv(batch * op->Ho * op->Wo, tile_bm(tile)) * walk_split(tile);   // one (or two) workgroups per pixel tile
      if (!is_im2col_tile(tile)) {
        if (int rc = launch_patch_grouped_tile<HT>(tile, gargs, n, (int)blocks, std::max(lds_max, op->min_lds), main_st)) return rc;
      } else if (int rc = launch_dma_grouped_tile<HT>(tile, gargs, n, (int)blocks, op->min_lds, main_st)) {
        return rc;
      }
      COMIC_LAUNCH_CHECK("grouped conv");
      gargs += n;
      i += n - 1;
      continue;
    }
    hipStream_t st = main_st;
    if (op->lane > 0) {
      COMIC_REQUIRE(lanes && op->lane <= 3, "branch lane %d outside a fork/join region", op->lane);
      st = lanes->s[op->lane - 1];
      used[op->lane - 1] = true;
    }
    if (op->kind == 8 || op->kind == 9) {
      // streaming Conv2d_2a -> Conv2d_2b -> MaxPool_3a (conv_stem.hip); weights[op->weight], [op->weight + 1].
      // kind 9: Conv2d_1a_3x3 inside the same pass -- src is the fp32 image (H, W = the image), the weight records are
      // Conv2d_1a (stem layout), Conv2d_2a, Conv2d_2b
      const bool with_1a = op->kind == 9;
      const int H0 = with_1a ? (op->H - 3) / 2 + 1 : op->H, W0 = with_1a ? (op->W - 3) / 2 + 1 : op->W;
      COMIC_REQUIRE(dtype == Half16<HT>::code && op->lane == 0, "stem stream: bf16 / f16 plans on the caller's stream only");
      COMIC_REQUIRE(op->Cin == (with_1a ? 3 : 32) && op->Cout == 64 && op->KH == 3 && op->KW == 3 && op->SH == 1 && op->SW == 1,
                    "stem stream: expects the (3 ->) 32 -> 32 -> 64 3x3 stem (got Cin %d, Cout %d)", op->Cin, op->Cout);
      COMIC_REQUIRE(comic_stem_stream_supported(H0, W0) && (!with_1a || comic_stem_stream_1a_supported(op->H, op->W)),
                    "stem stream: map %dx%d is not supported", op->H, op->W);
      const int Hp = (H0 - 2 - 3) / 2 + 1, Wp = (W0 - 2 - 3) / 2 + 1;
      COMIC_REQUIRE(op->Ho == Hp && op->Wo == Wp, "stem stream: Ho/Wo must be the pooled grid %dx%d", Hp, Wp);
      const comic_conv_weight* w0 = with_1a ? weights + op->weight : nullptr;
      const comic_conv_weight* wa = weights + op->weight + (with_1a ? 1 : 0);
      const comic_conv_weight* wb = wa + 1;
      const int xc = buf_channels[op->src], yc = buf_channels[op->dst];
      COMIC_REQUIRE(buffers[op->src] && buffers[op->dst] && wa->w && wb->w && wa->scale && wa->shift && wb->scale && wb->shift,
                    "stem stream: null buffer / weights");
      COMIC_REQUIRE(op->dst_coff + 64 <= yc && yc % 4 == 0 && op->dst_coff % 4 == 0, "stem stream: bad destination slice");
      COMIC_REQUIRE((long)batch * Hp * Wp * yc * 2 < (1L << 31), "stem stream: tensor too large");
      ComicStemArgs sa{};
      if (with_1a) {
        COMIC_REQUIRE(w0->w && w0->scale && w0->shift && xc == 3 && op->src_coff == 0, "stem stream: Conv2d_1a needs the whole fp32 image");
        sa.img = (const float*)buffers[op->src]; sa.Hi = op->H; sa.Wi = op->W;
        sa.w0 = (const float*)w0->w; sa.sc0 = w0->scale; sa.sh0 = w0->shift;
        sa.x = nullptr; sa.x_cs = 32; sa.x_co = 0;
      } else {
        COMIC_REQUIRE(op->src_coff + 32 <= xc && xc % 8 == 0 && op->src_coff % 8 == 0, "stem stream: bad source slice");
        COMIC_REQUIRE((long)batch * op->H * op->W * xc * 2 < (1L << 31), "stem stream: tensor too large");
        sa.x = (const bf16_t*)buffers[op->src]; sa.x_cs = xc; sa.x_co = op->src_coff;
      }
      sa.B = batch; sa.H0 = H0; sa.W0 = W0;
      sa.w1 = (const bf16_t*)wa->w; sa.w2 = (const bf16_t*)wb->w; sa.Kpad = (9 * 32 + 63) / 64 * 64;
      sa.sc1 = wa->scale; sa.sh1 = wa->shift; sa.sc2 = wb->scale; sa.sh2 = wb->shift;
      sa.y = (bf16_t*)buffers[op->dst]; sa.y_cs = yc; sa.y_co = op->dst_coff; sa.Hp = Hp; sa.Wp = Wp;
      sa.n_tasks = 2 * batch;
      sa.f16 = std::is_same<HT, f16_t>::value;
      if (int rc = comic_stem_stream_launch(sa, main_st)) return rc;
      COMIC_LAUNCH_CHECK("stem stream");
      continue;
    }
    const comic_conv_weight* wt = (op->kind <= 1 || op->kind == 7) ? weights + op->weight : nullptr;
    int rc = comic_conv2d_bn_relu(op, buffers[op->src], buf_channels[op->src], buffers[op->dst],
                                  buf_channels[op->dst], wt, batch, dtype, (void*)st);
    if (rc) return rc;
  }
  return 0;
}

extern "C" int comic_cnn_forward(const comic_cnn_op* ops, int n_ops, void* const* buffers, const int32_t* buf_channels,
                                 const comic_conv_weight* weights, int batch, int dtype, void* stream) {
  if (dtype == COMIC_F16) return cnn_forward_impl<f16_t>(ops, n_ops, buffers, buf_channels, weights, batch, dtype, nullptr, stream);
  return cnn_forward_impl<bf16_t>(ops, n_ops, buffers, buf_channels, weights, batch, dtype, nullptr, stream);
}

extern "C" int comic_cnn_forward_grouped(const comic_cnn_op* ops, int n_ops, void* const* buffers,
                                         const int32_t* buf_channels, const comic_conv_weight* weights, int batch,
                                         int dtype, const void* group_args_dev, void* stream) {
  COMIC_REQUIRE(group_args_dev || comic_cnn_group_args_bytes(ops, n_ops) == 0,
                "comic_cnn_forward_grouped: plan has grouped ops but no argument records");
  if (dtype == COMIC_F16)
    return cnn_forward_impl<f16_t>(ops, n_ops, buffers, buf_channels, weights, batch, dtype, group_args_dev, stream);
  return cnn_forward_impl<bf16_t>(ops, n_ops, buffers, buf_channels, weights, batch, dtype, group_args_dev, stream);
}

extern "C" int comic_pack_conv_weights(const float* w_hwio, void* w_packed, int kh, int kw, int cin, int cout,
                                       int dtype, void* stream) {
  const int K = kh * kw * cin, Kpad = (K + 63) / 64 * 64;
  const long total = (long)cout * Kpad;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == COMIC_BF16)
    hipLaunchKernelGGL((pack_conv_weights_kernel<bf16_t>), dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st,
                       w_hwio, (bf16_t*)w_packed, K, Kpad, cout);
  else if (dtype == COMIC_F16)
    hipLaunchKernelGGL((pack_conv_weights_kernel<f16_t>), dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st,
                       w_hwio, (f16_t*)w_packed, K, Kpad, cout);
  else
    hipLaunchKernelGGL((pack_conv_weights_kernel<float>), dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st,
                       w_hwio, (float*)w_packed, K, Kpad, cout);
  COMIC_LAUNCH_CHECK("pack_conv_weights");
  return 0;
}

extern "C" int comic_fold_bn(const float* beta, const float* mean, const float* var, float eps, float* scale,
                             float* shift, int c, void* stream) {
  hipLaunchKernelGGL(fold_bn_kernel, dim3(cdiv(c, 256)), dim3(256), 0, (hipStream_t)stream, beta, mean, var, eps,
                     scale, shift, c);
  COMIC_LAUNCH_CHECK("fold_bn");
  return 0;
}

// fp32 master -> plan-dtype copy of a flat parameter block (the packed layouts are identical)
namespace {
template <typename HT>
__global__ void f32_to_half_kernel(const float* __restrict__ in, HT* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = Half16<HT>::from_f32(in[i]);
}
__global__ void refold_bn_kernel(const float* __restrict__ beta, const float* __restrict__ mean,
                                 const float* __restrict__ scale, float* __restrict__ shift, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) shift[i] = beta[i] - mean[i] * scale[i];
}
}  // namespace

extern "C" int comic_cnn_refresh_weights_dtype(const float* master, void* plan_copy, int64_t n, const float* beta,
                                               const float* mean, const float* scale, float* shift, int64_t channels,
                                               int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  COMIC_REQUIRE(dtype == COMIC_BF16 || dtype == COMIC_F16, "cnn_refresh_weights: the plan copy is bf16 or f16 (got dtype %d)", dtype);
  if (plan_copy && n > 0) {
    COMIC_REQUIRE(master, "cnn_refresh_weights: null master");
    if (dtype == COMIC_F16)
      hipLaunchKernelGGL(f32_to_half_kernel<f16_t>, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, master, (f16_t*)plan_copy,
                         (long)n);
    else
      hipLaunchKernelGGL(f32_to_half_kernel<bf16_t>, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, master, (bf16_t*)plan_copy,
                         (long)n);
  }
  if (channels > 0) {
    COMIC_REQUIRE(beta && mean && scale && shift, "cnn_refresh_weights: null BN arrays");
    hipLaunchKernelGGL(refold_bn_kernel, dim3((unsigned)cdiv64(channels, 256)), dim3(256), 0, st, beta, mean, scale,
                       shift, (long)channels);
  }
  COMIC_LAUNCH_CHECK("cnn_refresh_weights");
  return 0;
}

extern "C" int comic_cnn_refresh_weights(const float* master, void* plan_copy, int64_t n, const float* beta,
                                         const float* mean, const float* scale, float* shift, int64_t channels,
                                         void* stream) {
  return comic_cnn_refresh_weights_dtype(master, plan_copy, n, beta, mean, scale, shift, channels, COMIC_BF16, stream);
}

#ifdef COMIC_STAMPS
extern "C" int comic_debug_read_stamps(unsigned long long* host, int n) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), (size_t)n * 8) == hipSuccess ? 0 : 1;
}
#endif
