// CNN encoder backward for gfx950 (the forward is conv.hip; conv_run.h is all the two files share).
#include "conv_run.h"
#include <algorithm>
#include <vector>

// =================================================================================================
// Backward of the plan (train_mode cnn_finetune, src/train.py:241-249): freeze_scopes == '' puts the
// conv weights and BN betas into the trainable set (src/model_base.py:834-849) while the graph stays
// in BN-inference mode (model_base.py:76), so per conv
//     z = conv(x, w) * scale + (beta - mean * scale),  y = relu(z)
//     dz = 1[y > 0] * dy ;  d beta = sum_pixels dz ;  d conv = dz * scale
//     d w = x^T (*) d conv (backward-weight) ;  d x += w^T (*) d conv (backward-data)
// Backward-data runs the FORWARD kernels on `d conv` with the flipped / transposed filter
// (stride-2 convs: `d conv` is written zero-dilated), accumulating into the gradient buffer.
// Backward-weight is an implicit GEMM whose reduction runs over output pixels; operand tiles are
// transposed on their way into LDS so the MFMA fragments are the same 16-byte row reads as in the
// forward kernel; pixel ranges are split over workgroups and combined with fp32 atomics.
// =================================================================================================
namespace {

template <typename T>
__device__ __forceinline__ void load_chunk_f(const void* base, size_t elem_off, bool f32, float* v) {
  constexpr int EPC = Elem<T>::EPC;
  if (sizeof(T) == 4 || f32) {
    const float* p = (const float*)base + elem_off;
#pragma unroll
    for (int i = 0; i < EPC; i += 4) {
      const float4 t = *(const float4*)(p + i);
      v[i] = t.x; v[i + 1] = t.y; v[i + 2] = t.z; v[i + 3] = t.w;
    }
  } else {
    load_vec<T>((const T*)base + elem_off, v);
  }
}
template <typename T>
__device__ __forceinline__ void store_chunk_f(void* base, size_t elem_off, bool f32, const float* v) {
  constexpr int EPC = Elem<T>::EPC;
  if (sizeof(T) == 4 || f32) {
    float* p = (float*)base + elem_off;
#pragma unroll
    for (int i = 0; i < EPC; i += 4) *(float4*)(p + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
  } else {
    store_vec<T>((T*)base + elem_off, v);
  }
}

struct ActGradArgs {
  const void* y;    // forward output (post-ReLU), channel slice [yco, yco + C) of rows of ycs channels
  const void* dy;   // its gradient, same geometry
  int ycs, yco, yf32;
  const float* scale;
  void* dz;         // [B][Hd][Wd][C] plan dtype; output pixel (ho, wo) lands at (ho*dil, wo*dil)
  int B, Ho, Wo, C, Hd, Wd, dil;
};

// grid (pixel chunks, ceil(C/64)); 256 threads = (64/EPC channel chunks) x (pixel lanes).  Besides dz
// the workgroup reduces its share of d beta[c] = sum_pixels 1[y>0] dy (unscaled) in LDS and adds
// it to the fp32 accumulator with one atomic per channel.
template <typename T>
__global__ __launch_bounds__(256) void act_grad_kernel(ActGradArgs a, float* __restrict__ dbeta, long px_per_block) {
  constexpr int EPC = Elem<T>::EPC;
  constexpr int CPB = 64 / EPC;        // channel chunks per workgroup
  constexpr int PL = 256 / CPB;        // pixel lanes
  __shared__ float red[PL][64 + 1];
  const int tid = threadIdx.x;
  const int cc = tid % CPB, pl = tid / CPB;
  const int c0 = blockIdx.y * 64 + cc * EPC;
  const bool cok = c0 < a.C;           // C % EPC == 0
  const long P = (long)a.B * a.Ho * a.Wo;
  const long p0 = (long)blockIdx.x * px_per_block, p1 = min(P, p0 + px_per_block);
  float sc[EPC], sum[EPC];
#pragma unroll
  for (int i = 0; i < EPC; ++i) {
    sc[i] = cok ? a.scale[c0 + i] : 0.f;
    sum[i] = 0.f;
  }
  if (cok) {
    for (long p = p0 + pl; p < p1; p += PL) {
      const int wo = (int)(p % a.Wo);
      const long q = p / a.Wo;
      const int ho = (int)(q % a.Ho), b = (int)(q / a.Ho);
      float yv[EPC], gv[EPC];
      const size_t src = (size_t)p * a.ycs + a.yco + c0;
      load_chunk_f<T>(a.y, src, a.yf32 != 0, yv);
      load_chunk_f<T>(a.dy, src, a.yf32 != 0, gv);
#pragma unroll
      for (int i = 0; i < EPC; ++i) {
        const float g = yv[i] > 0.f ? gv[i] : 0.f;
        sum[i] += g;
        gv[i] = g * sc[i];
      }
      const size_t dst = (((size_t)b * a.Hd + ho * a.dil) * a.Wd + wo * a.dil) * a.C + c0;
      store_chunk_f<T>(a.dz, dst, false, gv);
    }
  }
#pragma unroll
  for (int i = 0; i < EPC; ++i) red[pl][cc * EPC + i] = sum[i];
  __syncthreads();
  if (tid < 64) {
    const int c = blockIdx.y * 64 + tid;
    if (c < a.C) {
      float s = 0.f;
#pragma unroll 8
      for (int r = 0; r < PL; ++r) s += red[r][tid];
      atomicAdd(dbeta + c, s);
    }
  }
}

// The same for COMIC_OP_X3 plans (bf16x3 backward): y is hi + lo of two channel regions (or fp32), dy an fp32 gradient
// buffer of the LOGICAL channels, and dz leaves as the three regions [hi | lo | hi] of C channels each -- the operand
// layout of the x3 convolutions, so that the backward-data conv of dz against [Wt_hi | Wt_hi | Wt_lo] is the split product
// hi*hi + lo*hi + hi*lo with fp32 accumulation.
struct ActGradX3Args {
  const void* y;    // forward output: bf16 regions (hi at yco, lo y_lo channels behind) of rows of ycs channels, or fp32 (y_lo = 0)
  const float* dy;  // its gradient: fp32 rows of gcs channels, slice from yco
  int ycs, yco, y_lo, gcs;
  const float* scale;
  bf16_t* dz;       // [B][Hd][Wd][3 C]
  int B, Ho, Wo, C, Hd, Wd, dil;
};
__global__ __launch_bounds__(256) void act_grad_x3_kernel(ActGradX3Args a, float* __restrict__ dbeta, long px_per_block) {
  constexpr int EPC = 8, CPB = 64 / EPC, PL = 256 / CPB;
  __shared__ float red[PL][64 + 1];
  const int tid = threadIdx.x;
  const int cc = tid % CPB, pl = tid / CPB;
  const int c0 = blockIdx.y * 64 + cc * EPC;
  const bool cok = c0 < a.C;           // C % 8 == 0
  const long P = (long)a.B * a.Ho * a.Wo;
  const long p0 = (long)blockIdx.x * px_per_block, p1 = min(P, p0 + px_per_block);
  float sc[EPC], sum[EPC];
#pragma unroll
  for (int i = 0; i < EPC; ++i) {
    sc[i] = cok ? a.scale[c0 + i] : 0.f;
    sum[i] = 0.f;
  }
  if (cok) {
    for (long p = p0 + pl; p < p1; p += PL) {
      const int wo = (int)(p % a.Wo);
      const long q = p / a.Wo;
      const int ho = (int)(q % a.Ho), b = (int)(q / a.Ho);
      float yv[EPC], gv[EPC];
      const size_t src = (size_t)p * a.ycs + a.yco + c0;
      if (a.y_lo) {
        float yl[EPC];
        load_vec<bf16_t>((const bf16_t*)a.y + src, yv);
        load_vec<bf16_t>((const bf16_t*)a.y + src + a.y_lo, yl);
#pragma unroll
        for (int i = 0; i < EPC; ++i) yv[i] += yl[i];
      } else {
        load_chunk_f<bf16_t>(a.y, src, true, yv);
      }
      load_chunk_f<bf16_t>(a.dy, (size_t)p * a.gcs + a.yco + c0, true, gv);
      float hi[EPC], lo[EPC];
#pragma unroll
      for (int i = 0; i < EPC; ++i) {
        const float g = yv[i] > 0.f ? gv[i] : 0.f;
        sum[i] += g;
        {
          // z is the ROUNDED product, the value act_grad_kernel stores on the fp32 plan: contracted, z - hi becomes
          // fma(g, sc, -hi) and lo is the residue of another number
#pragma clang fp contract(off)
          const float z = g * sc[i];
          hi[i] = bf16_to_f32(f32_to_bf16(z));
          lo[i] = z - hi[i];
        }
      }
      bf16_t* dst = a.dz + (((size_t)b * a.Hd + ho * a.dil) * a.Wd + wo * a.dil) * 3 * a.C + c0;
      store_vec<bf16_t>(dst, hi);
      store_vec<bf16_t>(dst + a.C, lo);
      store_vec<bf16_t>(dst + 2 * a.C, hi);
    }
  }
#pragma unroll
  for (int i = 0; i < EPC; ++i) red[pl][cc * EPC + i] = sum[i];
  __syncthreads();
  if (tid < 64) {
    const int c = blockIdx.y * 64 + tid;
    if (c < a.C) {
      float s = 0.f;
#pragma unroll 8
      for (int r = 0; r < PL; ++r) s += red[r][tid];
      atomicAdd(dbeta + c, s);
    }
  }
}

// master [Cout][Kpad] (fp32, k = (kh*KW + kw)*Cin + ci) -> x3 backward-data filter [Cin][Kpad2], k2 = tap2 * 3 Cout + region * Cout +
// co with the flipped taps of pack_bwd_weights_kernel and the regions [W_hi | W_hi | W_lo]
__device__ __forceinline__ bf16_t pack_bwd_x3_value(const float* __restrict__ master, int k2, int ci, int KH, int KW, int Cin,
                                                    int Cout, int Kpad) {
  if (k2 >= KH * KW * 3 * Cout) return f32_to_bf16(0.f);
  const int tap2 = k2 / (3 * Cout), rr = k2 - tap2 * 3 * Cout;
  const int region = rr / Cout, co = rr - region * Cout;
  const int kh = KH - 1 - tap2 / KW, kw = KW - 1 - tap2 % KW;
  const float v = master[(size_t)co * Kpad + (kh * KW + kw) * Cin + ci];
  const bf16_t hi = f32_to_bf16(v);
  return region < 2 ? hi : f32_to_bf16(v - bf16_to_f32(hi));
}
__global__ void pack_bwd_weights_x3_kernel(const float* __restrict__ master, bf16_t* __restrict__ out, int KH, int KW, int Cin,
                                           int Cout, int Kpad, int Kpad2) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)Cin * Kpad2) return;
  out[idx] = pack_bwd_x3_value(master, (int)(idx % Kpad2), (int)(idx / Kpad2), KH, KW, Cin, Cout, Kpad);
}

// master [Cout][Kpad] (k = (kh*KW + kw)*Cin + ci) -> backward-data filter [Cin][Kpad2],
// k2 = ((KH-1-kh)*KW + (KW-1-kw))*Cout + co
template <typename T>
__global__ void pack_bwd_weights_kernel(const float* __restrict__ master, T* __restrict__ out, int KH, int KW, int Cin,
                                        int Cout, int Kpad, int Kpad2) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)Cin * Kpad2) return;
  const int k2 = (int)(idx % Kpad2), ci = (int)(idx / Kpad2);
  float v = 0.f;
  if (k2 < KH * KW * Cout) {
    const int tap2 = k2 / Cout, co = k2 % Cout;
    const int kh = KH - 1 - tap2 / KW, kw = KW - 1 - tap2 % KW;
    v = master[(size_t)co * Kpad + (kh * KW + kw) * Cin + ci];
  }
  if (sizeof(T) == 4)
    ((float*)out)[idx] = v;
  else
    ((bf16_t*)out)[idx] = f32_to_bf16(v);
}

struct WgradArgs {
  const void* dz;   // [B][Hd][Wd][dz_cs] plan dtype, channels [dz_co, dz_co + Cout) (plain plans: dz_cs = Cout, dz_co = 0)
  int Hd, Wd, dil, dz_cs, dz_co;
  int x_part;       // STEM, bf16: 0 the image rounded to bf16, 1 its rounding residue (the lo half of an x3 backward)
  int parts;        // 3: the x3 backward's three products in ONE launch -- blockIdx.z = split * 3 + part, part 0 (x hi, dz hi),
                    // 1 (x lo: x_lo_off channels further / the stem's residue, dz hi), 2 (x hi, dz lo: z_lo_off channels further)
  int x_lo_off, z_lo_off;
  const void* x;    // forward input (plan dtype; STEM: fp32 image)
  int x_cs, x_co;
  float* dw;        // [Cout][Kpad] fp32 (STEM: [K][Cout]), accumulated with atomics
  int B, H, W, Cin, Cout, KH, KW, SH, SW, PT, PL, Ho, Wo, K, Kpad;
  long P, p_per_split;
};

// grid (Kpad/64, ceil(Cout/64), splits): D[co][kk] += sum_{p in slice} dz[p][co] * xcol[p][kk]
template <typename T, bool STEM>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradArgs a) {
  constexpr int EPC = Elem<T>::EPC;
  constexpr int BKE = 4 * EPC;          // pixels per k-step (64 bytes of k per LDS row)
  constexpr int CPP = 64 / EPC;         // 16-byte chunks per pixel in a 64-channel tile
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 2 * 64 * kRowBytes];
  unsigned char* Zs = smem;                        // [2][64 co][kRowBytes]
  unsigned char* Xs = smem + 2 * 64 * kRowBytes;   // [2][64 kk][kRowBytes]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int kk0 = blockIdx.x * 64, co0 = blockIdx.y * 64;
  int bz = blockIdx.z;
  if (a.parts == 3) {
    const int part = bz % 3;
    bz /= 3;
    a.x_co += part == 1 ? a.x_lo_off : 0;
    a.x_part = part == 1;
    a.dz_co += part == 2 ? a.z_lo_off : 0;
  }
  const long p_begin = (long)bz * a.p_per_split, p_end = min(a.P, p_begin + a.p_per_split);
  const int px_l = tid / CPP, cg = tid % CPP;
  // this thread's fixed channel chunk of each tile
  const int co_c = co0 + cg * EPC;
  const bool co_ok = co_c < a.Cout;           // Cout % EPC == 0
  const int kk_c = kk0 + cg * EPC;
  int kh = 0, kw = 0, ci = 0;
  bool kk_ok = kk_c < a.K;
  if (!STEM) {
    if (kk_ok) {
      const int tap = kk_c / a.Cin;
      ci = kk_c % a.Cin;
      kh = tap / a.KW;
      kw = tap % a.KW;
    }
  }
  const int hw = a.Ho * a.Wo;
  uint4 zreg, xreg;
  const uint4 zero4 = make_uint4(0, 0, 0, 0);
  auto load_tile = [&](long pbase) {
    const long p = pbase + px_l;
    zreg = xreg = zero4;
    if (p >= p_end) return;
    const int b = (int)(p / hw);
    const int rem = (int)(p - (long)b * hw);
    const int ho = rem / a.Wo, wo = rem - ho * a.Wo;
    if (co_ok)
      zreg = *(const uint4*)((const T*)a.dz + (((size_t)b * a.Hd + ho * a.dil) * a.Wd + wo * a.dil) * a.dz_cs + a.dz_co + co_c);
    if (STEM) {
      float v[EPC];
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        const int kk = kk_c + e;
        v[e] = 0.f;
        if (kk < a.K) {
          const int tap = kk / a.Cin, c = kk - tap * a.Cin;
          const int hi = ho * a.SH - a.PT + tap / a.KW, wi = wo * a.SW - a.PL + tap % a.KW;
          if ((unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W)
            v[e] = ((const float*)a.x)[((size_t)(b * a.H + hi) * a.W + wi) * a.x_cs + a.x_co + c];
        }
      }
      if (sizeof(T) == 4) {
        xreg = make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
      } else {
        if (a.x_part) {
#pragma unroll
          for (int e = 0; e < EPC; ++e) v[e] -= bf16_to_f32(f32_to_bf16(v[e]));
        }
        xreg = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4 % EPC], v[5 % EPC]),
                          pack_bf16x2(v[6 % EPC], v[7 % EPC]));
      }
    } else if (kk_ok) {
      const int hi = ho * a.SH - a.PT + kh, wi = wo * a.SW - a.PL + kw;
      if ((unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W)
        xreg = *(const uint4*)((const T*)a.x + ((size_t)(b * a.H + hi) * a.W + wi) * a.x_cs + a.x_co + ci);
    }
  };
  // transposed store: element e of the chunk goes to row (cg*EPC + e), k position px_l
  auto store_tile = [&](int buf) {
    unsigned char* zb = Zs + buf * 64 * kRowBytes;
    unsigned char* xb = Xs + buf * 64 * kRowBytes;
    if (sizeof(T) == 4) {
      const uint32_t zu[4] = {zreg.x, zreg.y, zreg.z, zreg.w}, xu[4] = {xreg.x, xreg.y, xreg.z, xreg.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        *(uint32_t*)(zb + (cg * 4 + e) * kRowBytes + px_l * 4) = zu[e];
        *(uint32_t*)(xb + (cg * 4 + e) * kRowBytes + px_l * 4) = xu[e];
      }
    } else {
      const uint32_t zu[4] = {zreg.x, zreg.y, zreg.z, zreg.w}, xu[4] = {xreg.x, xreg.y, xreg.z, xreg.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint16_t zv = (uint16_t)(e & 1 ? zu[e >> 1] >> 16 : zu[e >> 1] & 0xFFFFu);
        const uint16_t xv = (uint16_t)(e & 1 ? xu[e >> 1] >> 16 : xu[e >> 1] & 0xFFFFu);
        *(uint16_t*)(zb + (cg * 8 + e) * kRowBytes + px_l * 2) = zv;
        *(uint16_t*)(xb + (cg * 8 + e) * kRowBytes + px_l * 2) = xv;
      }
    }
  };

  f32x4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const int frow = lane & 15, fchunk = lane >> 4;
  const int zoff = (wn * 32 + frow) * kRowBytes + fchunk * 16;
  const int xoff = (wm * 32 + frow) * kRowBytes + fchunk * 16;

  if (p_begin < p_end) {
    load_tile(p_begin);
    store_tile(0);
    __syncthreads();
    int buf = 0;
    for (long pb = p_begin; pb < p_end; pb += BKE, buf ^= 1) {
      const bool more = pb + BKE < p_end;
      if (more) load_tile(pb + BKE);
      uint4 zf[2], xf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) zf[i] = *(const uint4*)(Zs + buf * 64 * kRowBytes + zoff + i * 16 * kRowBytes);
#pragma unroll
      for (int j = 0; j < 2; ++j) xf[j] = *(const uint4*)(Xs + buf * 64 * kRowBytes + xoff + j * 16 * kRowBytes);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if constexpr (sizeof(T) == 2) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, zf[i]),
                                                                __builtin_bit_cast(bf16x8_t, xf[j]), acc[i][j], 0, 0, 0);
          } else {
            const f32x4_t zv = __builtin_bit_cast(f32x4_t, zf[i]);
            const f32x4_t xv = __builtin_bit_cast(f32x4_t, xf[j]);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(zv[0], xv[0], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(zv[1], xv[1], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(zv[2], xv[2], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(zv[3], xv[3], acc[i][j], 0, 0, 0);
          }
        }
      if (more) store_tile(buf ^ 1);
      __syncthreads();
    }
  }
  // D[co][kk]: lane holds co = .. + 4*(lane>>4) + reg, kk = .. + (lane & 15)
  const int kcol = lane & 15, cq = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kk = kk0 + wm * 32 + j * 16 + kcol;
      if (kk >= a.K) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + wn * 32 + i * 16 + cq + r;
        if (co >= a.Cout) continue;
        float* dst = STEM ? a.dw + (size_t)kk * a.Cout + co : a.dw + (size_t)co * a.Kpad + kk;
        atomicAdd(dst, acc[i][j][r]);
      }
    }
}

// bf16 fast path of the backward-weight product: operand tiles stay pixel-major in LDS (16-byte
// stores, no scalar transposition) and the MFMA fragments are gathered with the CDNA4 transposing
// read ds_read_b64_tr_b16 (4 pixel rows x 16 channels per 16-lane group, delivered channel-major).
// k index <-> pixel mapping of a 32-pixel step: k = 8g + e  <->  pixel 4*(g + 4*(e >> 2)) + (e & 3), the
// same for both operands, so that the two 16-lane groups of a 32-lane half touch 8 consecutive pixel
// rows; with a row stride of 32*odd bytes those are 64 distinct banks (conflict-free).
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(8))) short s16x8_t;

template <int BM, int BN>   // BM output channels x BN filter taps*channels per workgroup
__global__ __launch_bounds__(256) void conv_wgrad_tr_kernel(WgradArgs a) {
  constexpr int ZS = BM * 2 + 32, XS = BN * 2 + 32;       // LDS row strides in bytes (32 * odd)
  constexpr int ZCH = BM / 64, XCH = BN / 64;             // 16-byte chunks per thread per step
  constexpr int TM = BM / 32, TN = BN / 32;               // 16x16 tiles per wave (2 x 2 waves)
  static_assert((ZS / 32) % 2 == 1 && (XS / 32) % 2 == 1, "bank-conflict-free row strides");
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 32 * (ZS + XS)];
  unsigned char* Zs = smem;                    // [2][32 px][ZS]
  unsigned char* Xs = smem + 2 * 32 * ZS;      // [2][32 px][XS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int kk0 = blockIdx.x * BN, co0 = blockIdx.y * BM;
  int bz = blockIdx.z;
  if (a.parts == 3) {
    const int part = bz % 3;
    bz /= 3;
    a.x_co += part == 1 ? a.x_lo_off : 0;
    a.dz_co += part == 2 ? a.z_lo_off : 0;
  }
  const long p_begin = (long)bz * a.p_per_split, p_end = min(a.P, p_begin + a.p_per_split);
  const int px_l = tid >> 3, cg = tid & 7;     // pixel of the step, 8-channel chunk inside 64 channels
  // fixed channel chunks of this thread
  int co_c[ZCH];
  bool co_ok[ZCH];
#pragma unroll
  for (int i = 0; i < ZCH; ++i) {
    co_c[i] = co0 + i * 64 + cg * 8;
    co_ok[i] = co_c[i] < a.Cout;
  }
  int kh[XCH], kw[XCH], ci[XCH];
  bool kk_ok[XCH];
#pragma unroll
  for (int i = 0; i < XCH; ++i) {
    const int kk = kk0 + i * 64 + cg * 8;
    kk_ok[i] = kk < a.K;
    const int tap = kk_ok[i] ? kk / a.Cin : 0;
    ci[i] = kk_ok[i] ? kk % a.Cin : 0;
    kh[i] = tap / a.KW;
    kw[i] = tap % a.KW;
  }
  const int hw = a.Ho * a.Wo;
  uint4 zreg[ZCH], xreg[XCH];
  const uint4 zero4 = make_uint4(0, 0, 0, 0);
  auto load_tile = [&](long pbase) {
    const long p = pbase + px_l;
#pragma unroll
    for (int i = 0; i < ZCH; ++i) zreg[i] = zero4;
#pragma unroll
    for (int i = 0; i < XCH; ++i) xreg[i] = zero4;
    if (p >= p_end) return;
    const int b = (int)(p / hw);
    const int rem = (int)(p - (long)b * hw);
    const int ho = rem / a.Wo, wo = rem - ho * a.Wo;
    const bf16_t* zp = (const bf16_t*)a.dz + (((size_t)b * a.Hd + ho * a.dil) * a.Wd + wo * a.dil) * a.dz_cs + a.dz_co;
#pragma unroll
    for (int i = 0; i < ZCH; ++i)
      if (co_ok[i]) zreg[i] = *(const uint4*)(zp + co_c[i]);
#pragma unroll
    for (int i = 0; i < XCH; ++i) {
      const int hi = ho * a.SH - a.PT + kh[i], wi = wo * a.SW - a.PL + kw[i];
      if (kk_ok[i] && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W)
        xreg[i] = *(const uint4*)((const bf16_t*)a.x + ((size_t)(b * a.H + hi) * a.W + wi) * a.x_cs + a.x_co + ci[i]);
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < ZCH; ++i) *(uint4*)(Zs + (buf * 32 + px_l) * ZS + (i * 64 + cg * 8) * 2) = zreg[i];
#pragma unroll
    for (int i = 0; i < XCH; ++i) *(uint4*)(Xs + (buf * 32 + px_l) * XS + (i * 64 + cg * 8) * 2) = xreg[i];
  };
  f32x4_t acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  // transposing-read lane addressing: 16-lane group g, lane j = 4q + p supplies row q, columns 4p..4p+3
  const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  const uint32_t zs0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) unsigned char*)Zs);
  const uint32_t xs0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) unsigned char*)Xs);
  const uint32_t zlane = (4 * g + q) * ZS + (wn * (BM / 2) + 4 * pp) * 2;   // + 16*ZS for the second half
  const uint32_t xlane = (4 * g + q) * XS + (wm * (BN / 2) + 4 * pp) * 2;
  auto tr_read = [&](uint32_t addr) -> s16x4_t {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(uintptr_t)addr);
  };

  if (p_begin < p_end) {
    load_tile(p_begin);
    store_tile(0);
    __syncthreads();
    int buf = 0;
    for (long pb = p_begin; pb < p_end; pb += 32, buf ^= 1) {
      const bool more = pb + 32 < p_end;
      if (more) load_tile(pb + 32);
      const uint32_t zb = zs0 + buf * 32 * ZS + zlane, xb = xs0 + buf * 32 * XS + xlane;
      s16x8_t zf[TM], xf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const s16x4_t lo = tr_read(zb + i * 32), hi = tr_read(zb + i * 32 + 16 * ZS);
        zf[i] = (s16x8_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const s16x4_t lo = tr_read(xb + j * 32), hi = tr_read(xb + j * 32 + 16 * XS);
        xf[j] = (s16x8_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, zf[i]),
                                                              __builtin_bit_cast(bf16x8_t, xf[j]), acc[i][j], 0, 0, 0);
      if (more) store_tile(buf ^ 1);
      __syncthreads();
    }
  }
  const int kcol = lane & 15, cq = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int kk = kk0 + wm * (BN / 2) + j * 16 + kcol;
      if (kk >= a.K) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + wn * (BM / 2) + i * 16 + cq + r;
        if (co >= a.Cout) continue;
        atomicAdd(a.dw + (size_t)co * a.Kpad + kk, acc[i][j][r]);
      }
    }
}

struct PoolGradArgs {
  const void* x;    // forward input of the pool (max only)
  const void* dy;   // gradient of the pool output, slice [yco, yco + C) of ycs
  void* dx;         // gradient of the pool input, slice [xco, xco + C) of xcs  (accumulated)
  int xcs, xco, ycs, yco, dy_f32, dx_f32;
  int B, H, W, C, KH, KW, SH, SW, PT, PL, Ho, Wo;
  int dxcs, dxco;   // channel stride / offset of dx (plain plans: xcs, xco)
  int x_lo;         // x3 plans: x is hi + lo, the lo region x_lo channels behind the hi region (0: plain)
};

// MODE 0 max (first maximum in window scan order), 1 avg over valid taps, 2 plain mean over the
// KHxKW VALID window (the head's global pool).  Gather form: one thread per input pixel x chunk.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void pool_grad_kernel(PoolGradArgs a) {
  constexpr int EPC = Elem<T>::EPC;
  const int cvecs = a.C / EPC;
  const long total = (long)a.B * a.H * a.W * cvecs;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int cv = (int)(idx % cvecs);
  const long p = idx / cvecs;
  const int wi = (int)(p % a.W);
  const long q = p / a.W;
  const int hi = (int)(q % a.H), b = (int)(q / a.H);
  float g[EPC];
#pragma unroll
  for (int j = 0; j < EPC; ++j) g[j] = 0.f;
  // windows (ho, wo) that contain (hi, wi): ho*SH - PT <= hi < ho*SH - PT + KH
  const int ho_lo = max(0, (hi + a.PT - a.KH + a.SH) / a.SH), ho_hi = min(a.Ho - 1, (hi + a.PT) / a.SH);
  const int wo_lo = max(0, (wi + a.PL - a.KW + a.SW) / a.SW), wo_hi = min(a.Wo - 1, (wi + a.PL) / a.SW);
  for (int ho = ho_lo; ho <= ho_hi; ++ho)
    for (int wo = wo_lo; wo <= wo_hi; ++wo) {
      float dyv[EPC];
      load_chunk_f<T>(a.dy, ((size_t)(b * a.Ho + ho) * a.Wo + wo) * a.ycs + a.yco + cv * EPC, a.dy_f32 != 0, dyv);
      if (MODE == 0) {
        float best[EPC];
        int arg[EPC];
#pragma unroll
        for (int j = 0; j < EPC; ++j) { best[j] = -INFINITY; arg[j] = -1; }
        for (int kh = 0; kh < a.KH; ++kh) {
          const int h2 = ho * a.SH - a.PT + kh;
          if ((unsigned)h2 >= (unsigned)a.H) continue;
          for (int kw = 0; kw < a.KW; ++kw) {
            const int w2 = wo * a.SW - a.PL + kw;
            if ((unsigned)w2 >= (unsigned)a.W) continue;
            float v[EPC];
            const T* xp = (const T*)a.x + ((size_t)(b * a.H + h2) * a.W + w2) * a.xcs + a.xco + cv * EPC;
            load_vec<T>(xp, v);
            if (a.x_lo) {                          // (hi + lo is exact in fp32: the order pool_x3_kernel's pairs have)
              float vl[EPC];
              load_vec<T>(xp + a.x_lo, vl);
#pragma unroll
              for (int j = 0; j < EPC; ++j) v[j] += vl[j];
            }
#pragma unroll
            for (int j = 0; j < EPC; ++j)
              if (v[j] > best[j]) { best[j] = v[j]; arg[j] = h2 * a.W + w2; }
          }
        }
#pragma unroll
        for (int j = 0; j < EPC; ++j)
          if (arg[j] == hi * a.W + wi) g[j] += dyv[j];
      } else if (MODE == 1) {
        const int h0 = max(0, ho * a.SH - a.PT), h1 = min(a.H, ho * a.SH - a.PT + a.KH);
        const int w0 = max(0, wo * a.SW - a.PL), w1 = min(a.W, wo * a.SW - a.PL + a.KW);
        const float inv = 1.0f / (float)((h1 - h0) * (w1 - w0));
#pragma unroll
        for (int j = 0; j < EPC; ++j) g[j] += dyv[j] * inv;
      } else {
        const float inv = 1.0f / (float)(a.KH * a.KW);
#pragma unroll
        for (int j = 0; j < EPC; ++j) g[j] += dyv[j] * inv;
      }
    }
  const size_t off = (size_t)p * a.dxcs + a.dxco + cv * EPC;
  float old[EPC];
  load_chunk_f<T>(a.dx, off, a.dx_f32 != 0, old);
#pragma unroll
  for (int j = 0; j < EPC; ++j) old[j] += g[j];
  store_chunk_f<T>(a.dx, off, a.dx_f32 != 0, old);
}


// MaxPoolGrad of the 3x3 / stride-2 pools (MaxPool_3a / 5a and the pool branches of Mixed_6a / 7a; VALID or padded), tiled
// through the LDS.  The gather kernel above re-derives a window's arg-max once per input pixel it covers: up to four
// windows x nine 16-byte loads per thread -- 136 us per pool at 32 images (profiles/r05_finetune_lanes.txt: 6.5 % of the
// step's chain lane for two element-wise ops).  Here a workgroup owns a 16 x 16 tile of INPUT pixels and CG channel chunks:
//   1. the <= 19 x 19 input pixels its <= 9 x 9 windows read go to the LDS once (taps outside the image: -inf);
//   2. one thread per (window, chunk) finds the arg-max per channel -- FIRST maximum in (kh, kw) scan order, strict >, as
//      the gather kernel and TF's MaxPoolGrad -- and keeps (tap index per channel, the window's dy chunk) in the LDS;
//   3. one thread per (input pixel, chunk) adds the dy of its <= 4 windows whose arg-max it is, in (ho, wo) order, into dx.
// Same comparisons, same sums in the same order as pool_grad_kernel<T, 0>: identical bits.
constexpr int kMpgTile = 16, kMpgWin = kMpgTile / 2 + 1, kMpgX = 2 * kMpgWin + 1, kMpgCG = 4;
// X3 (COMIC_OP_X3 plans): x is hi + lo of two bf16 regions (a.x_lo apart), dy / dx fp32 buffers with their own strides.
template <typename T, bool X3 = false>
__global__ __launch_bounds__(256) void maxpool_grad_s2_kernel(PoolGradArgs a, int tiles_y, int tiles_x, int cgroups) {
  constexpr int EPC = Elem<T>::EPC;
  __shared__ uint4 xs[kMpgCG][kMpgX * kMpgX];                           // raw 16-byte chunks of the input pixels
  __shared__ uint4 xs_lo[X3 ? kMpgCG : 1][X3 ? kMpgX * kMpgX : 1];      // ... of their lo region
  __shared__ __attribute__((aligned(16))) float dys[kMpgCG][kMpgWin * kMpgWin][EPC];
  __shared__ __attribute__((aligned(8))) unsigned char args[kMpgCG][kMpgWin * kMpgWin][8];
  int bid = blockIdx.x;
  const int cgi = bid % cgroups; bid /= cgroups;
  const int tx = bid % tiles_x; bid /= tiles_x;
  const int ty = bid % tiles_y;
  const int b = bid / tiles_y;
  const int tid = threadIdx.x;
  const int cvecs = a.C / EPC;
  const int cv0 = cgi * kMpgCG, ncv = min(kMpgCG, cvecs - cv0);
  const int y0 = ty * kMpgTile, x0 = tx * kMpgTile;
  // windows that touch the tile: ho * 2 - PT <= y <= ho * 2 - PT + 2 for some y in [y0, y0 + 16)
  const int ho_lo = max(0, (y0 + a.PT - 1) >> 1), ho_hi = min(a.Ho - 1, (min(a.H, y0 + kMpgTile) - 1 + a.PT) >> 1);
  const int wo_lo = max(0, (x0 + a.PL - 1) >> 1), wo_hi = min(a.Wo - 1, (min(a.W, x0 + kMpgTile) - 1 + a.PL) >> 1);
  const int nho = ho_hi - ho_lo + 1, nwo = wo_hi - wo_lo + 1;        // <= kMpgWin each (may be <= 0 at a ragged edge)
  const int xr0 = 2 * ho_lo - a.PT, xc0 = 2 * wo_lo - a.PL;          // input pixel of LDS position (0, 0)
  const int nxr = 2 * nho + 1, nxc = 2 * nwo + 1;
  const bool any = nho > 0 && nwo > 0;
  const uint32_t ninf = sizeof(T) == 2 ? 0xFF80FF80u : 0xFF800000u;  // -inf in every element of a chunk
  if (any) {
    for (int i = tid; i < nxr * nxc * ncv; i += 256) {
      const int c = i % ncv, px = i / ncv;
      const int r = px / nxc, q = px - r * nxc;
      const int h = xr0 + r, w = xc0 + q;
      uint4 v = make_uint4(ninf, ninf, ninf, ninf), vl = make_uint4(0, 0, 0, 0);
      if ((unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W) {
        const T* xp = (const T*)a.x + ((size_t)(b * a.H + h) * a.W + w) * a.xcs + a.xco + (cv0 + c) * EPC;
        v = *(const uint4*)xp;
        if constexpr (X3) vl = *(const uint4*)(xp + a.x_lo);
      }
      xs[c][r * kMpgX + q] = v;
      if constexpr (X3) xs_lo[c][r * kMpgX + q] = vl;
    }
  }
  __syncthreads();
  if (any) {
    for (int i = tid; i < nho * nwo * ncv; i += 256) {
      const int c = i % ncv, wdx = i / ncv;
      const int wr = wdx / nwo, wq = wdx - wr * nwo;
      float best[EPC];
      uint32_t arg[EPC];
#pragma unroll
      for (int j = 0; j < EPC; ++j) { best[j] = -INFINITY; arg[j] = 255u; }
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          float v[EPC];
          load_vec<T>((const T*)&xs[c][(2 * wr + kh) * kMpgX + 2 * wq + kw], v);
          if constexpr (X3) {
            float vl[EPC];
            load_vec<T>((const T*)&xs_lo[c][(2 * wr + kh) * kMpgX + 2 * wq + kw], vl);
#pragma unroll
            for (int j = 0; j < EPC; ++j) v[j] += vl[j];
          }
#pragma unroll
          for (int j = 0; j < EPC; ++j)
            if (v[j] > best[j]) { best[j] = v[j]; arg[j] = kh * 3 + kw; }
        }
      float dyv[EPC];
      load_chunk_f<T>(a.dy, ((size_t)(b * a.Ho + ho_lo + wr) * a.Wo + wo_lo + wq) * a.ycs + a.yco + (cv0 + c) * EPC, a.dy_f32 != 0, dyv);
      const int slot = wr * kMpgWin + wq;
#pragma unroll
      for (int j = 0; j < EPC; j += 4) *(float4*)&dys[c][slot][j] = make_float4(dyv[j], dyv[j + 1], dyv[j + 2], dyv[j + 3]);
      uint32_t lo = 0, hi = 0;
#pragma unroll
      for (int j = 0; j < EPC; ++j) {
        if (j < 4) lo |= arg[j] << (8 * j); else hi |= arg[j] << (8 * (j - 4));
      }
      *(uint2*)args[c][slot] = make_uint2(lo, hi);
    }
  }
  __syncthreads();
  for (int i = tid; i < kMpgTile * kMpgTile * ncv; i += 256) {
    const int c = i % ncv, px = i / ncv;
    const int hi = y0 + px / kMpgTile, wi = x0 + px % kMpgTile;
    if (hi >= a.H || wi >= a.W) continue;
    float g[EPC];
#pragma unroll
    for (int j = 0; j < EPC; ++j) g[j] = 0.f;
    const int h_lo = max(0, (hi + a.PT - 1) >> 1), h_hi = min(a.Ho - 1, (hi + a.PT) >> 1);
    const int w_lo = max(0, (wi + a.PL - 1) >> 1), w_hi = min(a.Wo - 1, (wi + a.PL) >> 1);
    for (int ho = h_lo; ho <= h_hi; ++ho)
      for (int wo = w_lo; wo <= w_hi; ++wo) {
        const uint32_t mine = (uint32_t)((hi - (2 * ho - a.PT)) * 3 + (wi - (2 * wo - a.PL)));
        const int slot = (ho - ho_lo) * kMpgWin + (wo - wo_lo);
        const uint2 ab = *(const uint2*)args[c][slot];
        float dv[EPC];
#pragma unroll
        for (int j = 0; j < EPC; j += 4) {
          const float4 t = *(const float4*)&dys[c][slot][j];
          dv[j] = t.x; dv[j + 1] = t.y; dv[j + 2] = t.z; dv[j + 3] = t.w;
        }
#pragma unroll
        for (int j = 0; j < EPC; ++j) {
          const uint32_t aj = j < 4 ? (ab.x >> (8 * j)) & 255u : (ab.y >> (8 * (j - 4))) & 255u;
          if (aj == mine) g[j] += dv[j];
        }
      }
    const size_t off = ((size_t)(b * a.H + hi) * a.W + wi) * a.dxcs + a.dxco + (cv0 + c) * EPC;
    float old[EPC];
    load_chunk_f<T>(a.dx, off, a.dx_f32 != 0, old);
#pragma unroll
    for (int j = 0; j < EPC; ++j) old[j] += g[j];
    store_chunk_f<T>(a.dx, off, a.dx_f32 != 0, old);
  }
}

// workgroups per backward-weight launch that the pixel split aims for (every split adds one fp32
// atomic pass over the filter; fewer splits measured slower)
int wgrad_blocks_target() { return 1024; }

// bytes of a conv's (zero-dilated) d-conv tensor, and of the scratch a backward pass needs: the largest one, or -- when the
// weight gradients run on a lane of their own -- all of them side by side
size_t dz_bytes_of(const comic_cnn_op* op, int batch, size_t es) {
  const int Hd = (op->Ho - 1) * op->SH + 1;
  const int Wd = (op->Wo - 1) * op->SW + 1;
  const int regions = (op->flags & COMIC_OP_X3) ? 3 : 1;      // x3 plans: d conv as [hi | lo | hi]
  return ((size_t)batch * Hd * Wd * op->Cout * regions * es + 255) & ~(size_t)255;
}
// (the scheduled backward keeps kMaskCopies partial d beta rows per conv behind the d-conv slices: fused activation gradients)
size_t dbeta_partial_bytes(const comic_cnn_op* op) { return ((size_t)kMaskCopies * op->Cout * sizeof(float) + 255) & ~(size_t)255; }
int64_t backward_scratch_bytes(const comic_cnn_op* ops, int n_ops, int batch, size_t es, bool all) {
  size_t best = 0, sum = 0;
  for (int i = 0; i < n_ops; ++i) {
    if (ops[i].kind > 1) continue;
    const size_t dz = dz_bytes_of(ops + i, batch, es);
    best = std::max(best, dz);
    sum += dz + dbeta_partial_bytes(ops + i);
  }
  return (int64_t)(all ? sum : best);
}

// d beta[c] += the kMaskCopies partial sums of every conv whose activation gradient ran in a backward-data epilogue; one
// workgroup per conv, the entries as kernel arguments
constexpr int kFoldMax = 120;
struct DbetaFoldTable {
  struct {
    const float* part;
    float* dbeta;
    int C, pad;
  } e[kFoldMax];
  int n;
};
static_assert(sizeof(DbetaFoldTable) <= 4096, "kernel argument block");
__global__ __launch_bounds__(256) void dbeta_fold_kernel(const DbetaFoldTable tb) {
  const auto& en = tb.e[blockIdx.x];
  for (int c = threadIdx.x; c < en.C; c += blockDim.x) {
    float s = 0.f;
#pragma unroll 8
    for (int r = 0; r < kMaskCopies; ++r) s += en.part[(size_t)r * en.C + c];
    en.dbeta[c] += s;
  }
}

inline bool link_streams(hipStream_t from, hipStream_t to) {     // `to` waits for everything issued on `from` so far
  hipEvent_t ev;
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return false;
  const bool ok = hipEventRecord(ev, from) == hipSuccess && hipStreamWaitEvent(to, ev, 0) == hipSuccess;
  (void)hipEventDestroy(ev);
  return ok;
}

// The transposed (16-bit) weight-gradient kernel on filled arguments: tile form, pixel split and grid.  parts: 1, or the 3
// products of an x3 backward (a.parts == 3) -- three work items per (tile, pixel split), blockIdx.z = split * 3 + part.
void launch_wgrad_tr(WgradArgs a, int parts, hipStream_t st) {
  const bool big_m = a.Cout % 128 == 0, big_n = a.Kpad % 128 == 0 && a.K >= 256;
  const int bm = big_m ? 128 : 64, bn = big_n ? 128 : 64;
  const int tiles2 = cdiv(a.K, bn) * cdiv(a.Cout, bm) * parts;
  long S2 = std::max<long>(1, std::min<long>(wgrad_blocks_target() / tiles2, cdiv64(a.P, 32L * 8)));
  a.p_per_split = cdiv64(cdiv64(a.P, S2), 32) * 32;
  S2 = cdiv64(a.P, a.p_per_split);
  dim3 g2(cdiv(a.K, bn), cdiv(a.Cout, bm), (unsigned)(parts * S2));
  if (big_m && big_n)
    hipLaunchKernelGGL((conv_wgrad_tr_kernel<128, 128>), g2, dim3(256), 0, st, a);
  else if (big_m)
    hipLaunchKernelGGL((conv_wgrad_tr_kernel<128, 64>), g2, dim3(256), 0, st, a);
  else if (big_n)
    hipLaunchKernelGGL((conv_wgrad_tr_kernel<64, 128>), g2, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((conv_wgrad_tr_kernel<64, 64>), g2, dim3(256), 0, st, a);
}

// The op a backward-data launch runs on the forward kernels: a stride-1 conv of the (zero-dilated, Hd x Wd) d-conv tensor
// with the flipped / transposed filter, cin -> cout channels, into the source slice of `op`.
comic_cnn_op bwd_data_op(const comic_cnn_op* op, int Hd, int Wd, int cin, int cout, int flags, int out_f32, int tile) {
  comic_cnn_op t = *op;
  t.kind = 0;
  t.flags = flags;
  t.H = Hd; t.W = Wd; t.Cin = cin; t.Cout = cout; t.SH = t.SW = 1;
  t.PT = op->KH - 1 - op->PT; t.PL = op->KW - 1 - op->PL;
  t.Ho = op->H; t.Wo = op->W;
  t.src_coff = 0; t.dst_coff = op->src_coff; t.relu = 0; t.out_f32 = out_f32; t.tile = tile; t.group = 0; t.lane = 0;
  return t;
}

// One conv's weight gradient dw += x^T dz (the d-conv tensor dz as act_grad_kernel / a fused backward-data epilogue wrote it).
struct PendingWgrad {
  const comic_cnn_op* op;
  const void* x;
  int xc;
  const void* dz;
  const comic_conv_grad* gr;
};
template <typename T>
int launch_wgrad(const comic_cnn_op* op, const void* x, int xc, const void* dz, const comic_conv_grad* gr, int batch, hipStream_t st) {
  constexpr int EPC = Elem<T>::EPC;
  const bool stem = op->kind == 1;
  const int K = op->KH * op->KW * op->Cin, Kpad = (K + 63) / 64 * 64;
  const int dil = op->SH;
  const int Hd = (op->Ho - 1) * dil + 1, Wd = (op->Wo - 1) * dil + 1;
  {
    WgradArgs a{};
    a.dz_cs = op->Cout; a.dz_co = 0; a.x_part = 0;
    a.dz = dz; a.Hd = Hd; a.Wd = Wd; a.dil = dil; a.x = x; a.x_cs = xc; a.x_co = op->src_coff; a.dw = gr->dw;
    a.B = batch; a.H = op->H; a.W = op->W; a.Cin = op->Cin; a.Cout = op->Cout; a.KH = op->KH; a.KW = op->KW;
    a.SH = op->SH; a.SW = op->SW; a.PT = op->PT; a.PL = op->PL; a.Ho = op->Ho; a.Wo = op->Wo; a.K = K; a.Kpad = Kpad;
    a.P = (long)batch * op->Ho * op->Wo;
    constexpr int BKE = 4 * EPC;
    const int tiles = cdiv(K, 64) * cdiv(op->Cout, 64);
    // (stem: K = 27 taps x 32 channels = 864 sums that EVERY workgroup adds into -- 2048 pixel slices queue up at those
    // addresses: Conv2d_1a's weight gradient, the last launch of the backward, 178 -> ~100 us with a quarter of the slices)
    long S = std::max<long>(1, std::min<long>((stem ? 512 : 2048) / tiles, cdiv64(a.P, (long)BKE * 8)));
    a.p_per_split = cdiv64(cdiv64(a.P, S), BKE) * BKE;
    S = cdiv64(a.P, a.p_per_split);
    dim3 grid(cdiv(K, 64), cdiv(op->Cout, 64), (unsigned)S);
    if (stem) {
      COMIC_REQUIRE(op->Cin <= 4, "stem conv backward: needs Cin <= 4");
      hipLaunchKernelGGL((conv_wgrad_kernel<T, true>), grid, dim3(256), 0, st, a);
    } else {
      COMIC_REQUIRE(op->Cin % EPC == 0 && op->src_coff % EPC == 0 && xc % EPC == 0, "conv backward: misaligned input slice");
      if constexpr (sizeof(T) == 2) {
        launch_wgrad_tr(a, 1, st);
      } else {
        hipLaunchKernelGGL((conv_wgrad_kernel<T, false>), grid, dim3(256), 0, st, a);
      }
    }
  }
  return 0;
}

template <typename T>
int conv_backward(const comic_cnn_op* op, const void* x, int xc, const void* y, const void* gy, int yc, void* gx,
                  const comic_conv_weight* wt, const comic_conv_grad* gr, int batch, void* scratch,
                  int64_t scratch_bytes, hipStream_t st, bool filters_ready, hipStream_t st_w,
                  bool dz_ready = false, const ConvMask* fuse = nullptr, std::vector<PendingWgrad>* defer = nullptr) {
  // dz_ready: the backward-data launch of this conv's only reader has written dz and added d beta (its epilogue applied this
  // conv's activation gradient); fuse: this conv's backward-data result is the gradient at the output of a conv with no
  // other reader -- apply that conv's activation gradient in the epilogue and write its dz instead of accumulating into gx.
  constexpr int EPC = Elem<T>::EPC;
  const bool stem = op->kind == 1;
  COMIC_REQUIRE(wt && wt->scale && gr && gr->w_master && gr->dw && gr->dbeta, "conv backward: missing weight / gradient record");
  COMIC_REQUIRE(op->Cout % EPC == 0 && op->dst_coff % EPC == 0 && yc % EPC == 0, "conv backward: misaligned output slice");
  COMIC_REQUIRE(op->SH == op->SW && (op->SH == 1 || op->SH == 2), "conv backward: stride must be 1 or 2");
  // what the launches below require of the conv is checked in front of the first of them, so a refused call leaves dw,
  // d beta and gx as they were: the weight gradient's input slice, and for the backward-data convolution the conditions of
  // the forward kernels it runs on (comic_run_op, with Cin in the place of Cout)
  if (stem) {
    COMIC_REQUIRE(op->Cin <= 4, "stem conv backward: needs Cin <= 4");
  } else {
    COMIC_REQUIRE(op->Cin % EPC == 0 && op->src_coff % EPC == 0 && xc % EPC == 0, "conv backward: misaligned input slice");
    if (gx || fuse) {
      COMIC_REQUIRE(gr->w_bwd, "conv backward: missing backward-data filter buffer");
      COMIC_REQUIRE(op->Cin % 16 == 0 && op->src_coff % 4 == 0 && xc % 4 == 0 && op->src_coff + op->Cin <= xc,
                    "conv backward: the backward-data convolution needs Cin %% 16 == 0 (got %d) and its slice inside the %d "
                    "channels of the source", op->Cin, xc);
    }
  }
  const int K = op->KH * op->KW * op->Cin, Kpad = (K + 63) / 64 * 64;
  const int dil = op->SH;
  // zero-dilated d conv geometry: output pixel (ho, wo) sits at (ho*dil, wo*dil); the backward-data
  // conv pads PT' = KH - 1 - PT rows on top and reads zeros below the buffer (bounds checks)
  const int Hd = (op->Ho - 1) * dil + 1;
  const int Wd = (op->Wo - 1) * dil + 1;
  const size_t dz_bytes = ((size_t)batch * Hd * Wd * op->Cout * sizeof(T) + 255) & ~(size_t)255;
  COMIC_REQUIRE((int64_t)dz_bytes <= scratch_bytes, "conv backward: scratch too small (%zu needed)", dz_bytes);
  T* dz = (T*)scratch;
  COMIC_REQUIRE(!dz_ready || dil == 1, "conv backward: a fused activation gradient writes an undilated d-conv tensor");
  if (dil > 1) {
    COMIC_REQUIRE(hipMemsetAsync(dz, 0, dz_bytes, st) == hipSuccess, "conv backward: memset failed");
  }
  if (!dz_ready) {
    ActGradArgs a{y, gy, yc, op->dst_coff, op->out_f32, wt->scale, dz, batch, op->Ho, op->Wo, op->Cout, Hd, Wd, dil};
    const long P = (long)batch * op->Ho * op->Wo;
    const long ppb = std::max<long>(64, cdiv64(P, 512));
    hipLaunchKernelGGL((act_grad_kernel<T>), dim3((unsigned)cdiv64(P, ppb), cdiv(op->Cout, 64)), dim3(256), 0, st, a,
                       gr->dbeta, ppb);
  }
  if (defer) {            // the caller launches the weight gradient later (launch_wgrad), behind one fork for several convs
    defer->push_back(PendingWgrad{op, x, xc, (const void*)dz, gr});
  } else {
    // the weight gradient runs on its own lane, beside the backward-data chain (dz is this conv's own)
    if (st_w != st) COMIC_REQUIRE(link_streams(st, st_w), "conv backward: fork of the weight-gradient lane failed");
    if (int rc = launch_wgrad<T>(op, x, xc, dz, gr, batch, st_w)) return rc;
  }
  COMIC_LAUNCH_CHECK("conv backward (weights)");
  if (stem || (!gx && !fuse)) return 0;
  // backward-data: forward conv of dz with the flipped / transposed filter, accumulated into gx
  COMIC_REQUIRE(gr->w_bwd, "conv backward: missing backward-data filter buffer");
  const int K2 = op->KH * op->KW * op->Cout, Kpad2 = (K2 + 63) / 64 * 64;
  if (!filters_ready) {
    const long n = (long)op->Cin * Kpad2;
    hipLaunchKernelGGL((pack_bwd_weights_kernel<T>), dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, gr->w_master,
                       (T*)gr->w_bwd, op->KH, op->KW, op->Cin, op->Cout, Kpad, Kpad2);
  }
  comic_cnn_op t = bwd_data_op(op, Hd, Wd, op->Cout, op->Cin, op->flags, /*out_f32=*/0, gr->bwd_tile);
  comic_conv_weight w2{gr->w_bwd, nullptr, nullptr};
  if (fuse) {
    t.dst_coff = 0;
    return comic_run_op<T>(&t, dz, op->Cout, fuse->dz, op->Cin, &w2, batch, st, /*accum=*/0, fuse);
  }
  return comic_run_op<T>(&t, dz, op->Cout, gx, xc, &w2, batch, st, /*accum=*/1);
}

// A conv of a COMIC_OP_X3 plan ("bf16x3": cnn_finetune at fp32-class accuracy on the bf16 matrix cores).  Activations are
// the three bf16 regions [hi | lo | hi] (xc, yc: physical channels = 3 x logical; fp32 outputs as they are), gradient
// buffers fp32 of the LOGICAL channels (gxc, gyc), masters and weight gradients the logical [Cout][Kpad] of the bf16 plan.
//   dz  = 1[y > 0] dy scale as [hi | lo | hi]                                              (act_grad_x3_kernel)
//   dw += x_hi^T dz_hi + x_lo^T dz_hi + x_hi^T dz_lo      one launch of the bf16 backward-weight kernel, three work items per
//                                                         (tile, pixel split) over channel slices of the regions, fp32
//                                                         atomics into the one dw
//   gx += conv(dz, [Wt_hi | Wt_hi | Wt_lo])               the bf16 forward kernels over 3 Cout channels, fp32 accumulate
int conv_backward_x3(const comic_cnn_op* op, const void* x, int xc, const void* y, const float* gy, int yc, int gyc, float* gx,
                     int gxc, const comic_conv_weight* wt, const comic_conv_grad* gr, int batch, void* scratch,
                     int64_t scratch_bytes, hipStream_t st, bool filters_ready, hipStream_t st_w) {
  const bool stem = op->kind == 1;
  COMIC_REQUIRE(wt && wt->scale && gr && gr->w_master && gr->dw && gr->dbeta, "conv backward (x3): missing weight / gradient record");
  COMIC_REQUIRE(op->SH == op->SW && (op->SH == 1 || op->SH == 2), "conv backward (x3): stride must be 1 or 2");
  COMIC_REQUIRE(op->Cout % 8 == 0 && op->dst_coff % 8 == 0 && (stem || (op->Cin % 3 == 0 && xc % 3 == 0)) &&
                    (op->out_f32 || yc % 3 == 0), "conv backward (x3): channel regions do not fit the buffers");
  const int cin = stem ? op->Cin : op->Cin / 3, x_lo = stem ? 0 : xc / 3, y_lo = op->out_f32 ? 0 : yc / 3;
  // (as in conv_backward: every refusal in front of the first launch)
  if (stem) {
    COMIC_REQUIRE(op->Cin <= 4, "stem conv backward: needs Cin <= 4");
  } else {
    COMIC_REQUIRE(cin % 8 == 0 && op->src_coff % 8 == 0 && x_lo % 8 == 0, "conv backward (x3): misaligned input slice");
    if (gx) {
      COMIC_REQUIRE(gr->w_bwd, "conv backward (x3): missing backward-data filter buffer");
      COMIC_REQUIRE(cin % 16 == 0 && op->src_coff % 4 == 0 && gxc % 4 == 0 && op->src_coff + cin <= gxc,
                    "conv backward (x3): the backward-data convolution needs Cin %% 16 == 0 (got %d) and its slice inside the "
                    "%d channels of the source gradient", cin, gxc);
    }
  }
  const int K = op->KH * op->KW * cin, Kpad = (K + 63) / 64 * 64;
  const int dil = op->SH;
  const int Hd = (op->Ho - 1) * dil + 1, Wd = (op->Wo - 1) * dil + 1;
  const size_t dz_bytes = dz_bytes_of(op, batch, 2);
  COMIC_REQUIRE((int64_t)dz_bytes <= scratch_bytes, "conv backward (x3): scratch too small (%zu needed)", dz_bytes);
  bf16_t* dz = (bf16_t*)scratch;
  if (dil > 1) COMIC_REQUIRE(hipMemsetAsync(dz, 0, dz_bytes, st) == hipSuccess, "conv backward (x3): memset failed");
  {
    ActGradX3Args a{y, gy, yc, op->dst_coff, y_lo, gyc, wt->scale, dz, batch, op->Ho, op->Wo, op->Cout, Hd, Wd, dil};
    const long P = (long)batch * op->Ho * op->Wo;
    const long ppb = std::max<long>(64, cdiv64(P, 512));
    hipLaunchKernelGGL(act_grad_x3_kernel, dim3((unsigned)cdiv64(P, ppb), cdiv(op->Cout, 64)), dim3(256), 0, st, a, gr->dbeta, ppb);
  }
  if (st_w != st) COMIC_REQUIRE(link_streams(st, st_w), "conv backward (x3): fork of the weight-gradient lane failed");
  {
    WgradArgs a{};
    a.dz = dz; a.Hd = Hd; a.Wd = Wd; a.dil = dil; a.dz_cs = 3 * op->Cout; a.x = x; a.x_cs = xc; a.dw = gr->dw;
    a.B = batch; a.H = op->H; a.W = op->W; a.Cin = cin; a.Cout = op->Cout; a.KH = op->KH; a.KW = op->KW;
    a.SH = op->SH; a.SW = op->SW; a.PT = op->PT; a.PL = op->PL; a.Ho = op->Ho; a.Wo = op->Wo; a.K = K; a.Kpad = Kpad;
    a.P = (long)batch * op->Ho * op->Wo;
    // the three products (x hi, dz hi), (x lo, dz hi), (x hi, dz lo) in one launch: blockIdx.z = split * 3 + part
    a.parts = 3; a.dz_co = 0; a.x_co = op->src_coff; a.x_part = 0; a.x_lo_off = x_lo; a.z_lo_off = op->Cout;
    if (stem) {
      COMIC_REQUIRE(op->Cin <= 4, "stem conv backward: needs Cin <= 4");
      const int tiles = cdiv(K, 64) * cdiv(op->Cout, 64) * 3;
      long S = std::max<long>(1, std::min<long>(2048 / tiles, cdiv64(a.P, 32L * 8)));
      a.p_per_split = cdiv64(cdiv64(a.P, S), 32) * 32;
      S = cdiv64(a.P, a.p_per_split);
      hipLaunchKernelGGL((conv_wgrad_kernel<bf16_t, true>), dim3(cdiv(K, 64), cdiv(op->Cout, 64), (unsigned)(3 * S)), dim3(256), 0,
                         st_w, a);
    } else {
      COMIC_REQUIRE(cin % 8 == 0 && op->src_coff % 8 == 0 && x_lo % 8 == 0, "conv backward (x3): misaligned input slice");
      launch_wgrad_tr(a, 3, st_w);
    }
  }
  COMIC_LAUNCH_CHECK("conv backward (x3, weights)");
  if (stem || !gx) return 0;
  COMIC_REQUIRE(gr->w_bwd, "conv backward (x3): missing backward-data filter buffer");
  const int K2 = op->KH * op->KW * 3 * op->Cout, Kpad2 = (K2 + 63) / 64 * 64;
  if (!filters_ready) {
    const long n = (long)cin * Kpad2;
    hipLaunchKernelGGL(pack_bwd_weights_x3_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, gr->w_master,
                       (bf16_t*)gr->w_bwd, op->KH, op->KW, cin, op->Cout, Kpad, Kpad2);
  }
  const comic_cnn_op t = bwd_data_op(op, Hd, Wd, 3 * op->Cout, cin, COMIC_OP_RAW, /*out_f32=*/1, /*tile=*/0);
  comic_conv_weight w2{gr->w_bwd, nullptr, nullptr};
  return comic_run_op<bf16_t>(&t, dz, 3 * op->Cout, gx, gxc, &w2, batch, st, /*accum=*/1);
}

// x3: the pool of a COMIC_OP_X3 plan -- x the bf16 regions (hi + lo), gy / gx fp32 buffers of the logical channels
template <typename T>
int pool_backward(const comic_cnn_op* op, const void* x, int xc, const void* gy, int yc, void* gx, int batch,
                  hipStream_t st, bool x3 = false) {
  constexpr int EPC = Elem<T>::EPC;
  COMIC_REQUIRE(op->Cin % EPC == 0 && op->src_coff % EPC == 0 && op->dst_coff % EPC == 0 && xc % EPC == 0 &&
                    yc % EPC == 0, "pool backward: misaligned channel slices");
  PoolGradArgs a{x, gy, gx, xc, op->src_coff, yc, op->dst_coff, op->kind == 4 ? 1 : 0,
                 (op->kind == 4 && op->src_f32) ? 1 : 0,
                 batch, op->H, op->W, op->Cin, op->KH, op->KW, op->SH, op->SW, op->PT, op->PL, op->Ho, op->Wo};
  a.dxcs = a.xcs; a.dxco = a.xco; a.x_lo = 0;
  if (x3) {
    COMIC_REQUIRE(sizeof(T) == 2 && xc % 3 == 0 && yc % 3 == 0 && (xc / 3) % EPC == 0 && (yc / 3) % EPC == 0,
                  "pool backward (x3): channel regions do not fit the buffers");
    a.x_lo = xc / 3; a.dxcs = xc / 3; a.ycs = yc / 3; a.dy_f32 = 1; a.dx_f32 = 1;
  }
  const long total = (long)batch * op->H * op->W * (op->Cin / EPC);
  dim3 grid((unsigned)cdiv64(total, 256));
  if (op->kind == 2 && op->KH == 3 && op->KW == 3 && op->SH == 2 && op->SW == 2 && op->PT >= 0 && op->PT <= 1 && op->PL >= 0 &&
      op->PL <= 1) {
    const int tiles_y = cdiv(op->H, kMpgTile), tiles_x = cdiv(op->W, kMpgTile), cgroups = cdiv(op->Cin / EPC, kMpgCG);
    const long wgs = (long)batch * tiles_y * tiles_x * cgroups;
    COMIC_REQUIRE(wgs < (1L << 31), "pool backward: too many tiles");
    if constexpr (sizeof(T) == 2) {
      if (x3) hipLaunchKernelGGL((maxpool_grad_s2_kernel<T, true>), dim3((unsigned)wgs), dim3(256), 0, st, a, tiles_y, tiles_x, cgroups);
      else hipLaunchKernelGGL((maxpool_grad_s2_kernel<T>), dim3((unsigned)wgs), dim3(256), 0, st, a, tiles_y, tiles_x, cgroups);
    } else {
      hipLaunchKernelGGL((maxpool_grad_s2_kernel<T>), dim3((unsigned)wgs), dim3(256), 0, st, a, tiles_y, tiles_x, cgroups);
    }
  } else if (op->kind == 2)
    hipLaunchKernelGGL((pool_grad_kernel<T, 0>), grid, dim3(256), 0, st, a);
  else if (op->kind == 3)
    hipLaunchKernelGGL((pool_grad_kernel<T, 1>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((pool_grad_kernel<T, 2>), grid, dim3(256), 0, st, a);
  COMIC_LAUNCH_CHECK("pool backward");
  return 0;
}

// Every conv of a plan in ONE launch (the entries travel as kernel arguments): 93 launches of 5 us each cost the host thread
// 0.63 ms per cnn_finetune step -- the next forward's first launch queued behind them -- for 0.4 ms of device work.
constexpr int kPackTableMax = 96;
struct PackBwdEntry {
  const float* master;
  void* out;
  uint32_t first_block;            // of this entry in the launch (entries ascending)
  uint16_t Cin, Cout;
  uint8_t KH, KW;
  uint8_t x3;                      // 1: [W_hi | W_hi | W_lo] regions per tap (Cin = channels of ONE source region)
  uint8_t pad[5];
};
struct PackBwdTable {
  PackBwdEntry e[kPackTableMax];
  int n;
};
static_assert(sizeof(PackBwdTable) <= 4096, "kernel argument block");

template <typename T>
__global__ __launch_bounds__(256) void pack_bwd_weights_table_kernel(const PackBwdTable tb) {
  int lo = 0, hi = tb.n - 1;                             // the entry this block belongs to
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tb.e[mid].first_block <= blockIdx.x) lo = mid;
    else hi = mid - 1;
  }
  const PackBwdEntry& en = tb.e[lo];
  const int KH = en.KH, KW = en.KW, Cin = en.Cin, Cout = en.Cout;
  const int Kpad = (KH * KW * Cin + 63) / 64 * 64, Kpad2 = (KH * KW * Cout * (en.x3 ? 3 : 1) + 63) / 64 * 64;
  const long idx = (long)(blockIdx.x - en.first_block) * blockDim.x + threadIdx.x;
  if (idx >= (long)Cin * Kpad2) return;
  if (en.x3) {
    if constexpr (sizeof(T) == 2)
      ((bf16_t*)en.out)[idx] = pack_bwd_x3_value(en.master, (int)(idx % Kpad2), (int)(idx / Kpad2), KH, KW, Cin, Cout, Kpad);
    return;
  }
  const int k2 = (int)(idx % Kpad2), ci = (int)(idx / Kpad2);
  float v = 0.f;
  if (k2 < KH * KW * Cout) {
    const int tap2 = k2 / Cout, co = k2 % Cout;
    const int kh = KH - 1 - tap2 / KW, kw = KW - 1 - tap2 % KW;
    v = en.master[(size_t)co * Kpad + (kh * KW + kw) * Cin + ci];
  }
  if (sizeof(T) == 4)
    ((float*)en.out)[idx] = v;
  else
    ((bf16_t*)en.out)[idx] = f32_to_bf16(v);
}

template <typename T>
int pack_bwd_filters_impl(const comic_cnn_op* ops, int n_ops, const comic_conv_grad* grads, hipStream_t st) {
  PackBwdTable tb;
  tb.n = 0;
  uint32_t blocks = 0;
  auto flush = [&]() {
    if (tb.n) hipLaunchKernelGGL((pack_bwd_weights_table_kernel<T>), dim3(blocks), dim3(256), 0, st, tb);
    tb.n = 0;
    blocks = 0;
  };
  for (int i = 0; i < n_ops; ++i) {
    const comic_cnn_op* op = ops + i;
    if (op->kind != 0) continue;
    const comic_conv_grad* gr = grads + op->weight;
    COMIC_REQUIRE(gr->w_master && gr->w_bwd, "pack_bwd_filters: missing buffers for conv %d", i);
    COMIC_REQUIRE(op->KH <= 255 && op->KW <= 255 && op->Cin <= 65535 && op->Cout <= 65535, "pack_bwd_filters: conv %d too large", i);
    const bool x3 = (op->flags & COMIC_OP_X3) != 0;
    COMIC_REQUIRE(!x3 || (sizeof(T) == 2 && op->Cin % 3 == 0), "pack_bwd_filters: COMIC_OP_X3 is a bf16-plan layout");
    const int cin = x3 ? op->Cin / 3 : op->Cin;
    const int K2 = op->KH * op->KW * op->Cout * (x3 ? 3 : 1), Kpad2 = (K2 + 63) / 64 * 64;
    const long n = (long)cin * Kpad2;
    if (tb.n == kPackTableMax) flush();
    PackBwdEntry& en = tb.e[tb.n++];
    en.master = gr->w_master;
    en.out = gr->w_bwd;
    en.first_block = blocks;
    en.x3 = x3 ? 1 : 0;
    en.Cin = (uint16_t)cin;
    en.Cout = (uint16_t)op->Cout;
    en.KH = (uint8_t)op->KH;
    en.KW = (uint8_t)op->KW;
    blocks += (uint32_t)cdiv64(n, 256);
  }
  flush();
  COMIC_LAUNCH_CHECK("pack_bwd_filters");
  return 0;
}

// forward filters of a COMIC_OP_X3 plan from the masters, every conv in one launch (comic_cnn_pack_x3_weights)
struct PackX3Entry {
  const float* master;
  bf16_t* out;
  uint32_t first_block;
  uint16_t cout, cin, taps, pad;
};
struct PackX3Table {
  PackX3Entry e[kPackTableMax];
  int n;
};
static_assert(sizeof(PackX3Table) <= 4096, "kernel argument block");
__global__ __launch_bounds__(256) void pack_x3_table_kernel(const PackX3Table tb) {
  int lo = 0, hi = tb.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tb.e[mid].first_block <= blockIdx.x) lo = mid;
    else hi = mid - 1;
  }
  const PackX3Entry& en = tb.e[lo];
  const int cin = en.cin, K = en.taps * cin, kpad = (K + 63) / 64 * 64, kpad3 = (3 * K + 63) / 64 * 64;
  const long idx = (long)(blockIdx.x - en.first_block) * blockDim.x + threadIdx.x;
  if (idx >= (long)en.cout * kpad3) return;
  const int k3 = (int)(idx % kpad3), row = (int)(idx / kpad3);
  bf16_t o = f32_to_bf16(0.f);
  if (k3 < 3 * K) {
    const int tap = k3 / (3 * cin), rr = k3 - tap * 3 * cin;
    const int region = rr / cin, ci = rr - region * cin;
    const float v = en.master[(size_t)row * kpad + tap * cin + ci];
    const bf16_t h = f32_to_bf16(v);
    o = region < 2 ? h : f32_to_bf16(v - bf16_to_f32(h));
  }
  en.out[idx] = o;
}

template <typename T>
int cnn_backward_impl(const comic_cnn_op* ops, int n_ops, void* const* buffers, void* const* grad_buffers,
                      const int32_t* buf_channels, const comic_conv_weight* weights, const comic_conv_grad* grads,
                      int batch, void* scratch, int64_t scratch_bytes, hipStream_t st, bool filters_ready,
                      hipStream_t st_w) {
  // Two lanes (st_w != st): every conv gets its own d-conv slice of the scratch, so its weight gradient (st_w) only
  // waits for its act_grad launch and runs beside the act_grad / backward-data chain of the earlier layers (st).
  const int64_t all = backward_scratch_bytes(ops, n_ops, batch, sizeof(T), true);
  if (st_w == nullptr || all > scratch_bytes) st_w = st;
  size_t dz_off = 0;
  for (int i = n_ops - 1; i >= 0; --i) {
    const comic_cnn_op* op = ops + i;
    if (op->kind == 5 || op->kind == 6) continue;
    void* gy = grad_buffers[op->dst];
    COMIC_REQUIRE(gy, "cnn_backward: op %d has no output gradient buffer", i);
    void* gx = grad_buffers[op->src];
    const int xc = buf_channels[op->src], yc = buf_channels[op->dst];
    const bool x3 = (op->flags & COMIC_OP_X3) != 0;
    if (x3 && op->kind <= 1) {
      if constexpr (sizeof(T) == 2) {
        const size_t dzb = dz_bytes_of(op, batch, sizeof(T));
        void* dz = st_w != st ? (void*)((char*)scratch + dz_off) : scratch;
        if (int rc = conv_backward_x3(op, buffers[op->src], xc, buffers[op->dst], (const float*)gy, yc, op->out_f32 ? yc : yc / 3,
                                      (float*)gx, op->kind == 1 ? 0 : xc / 3, weights + op->weight, grads + op->weight, batch, dz,
                                      st_w != st ? (int64_t)dzb : scratch_bytes, st, filters_ready, st_w))
          return rc;
        dz_off += dzb;
      } else {
        COMIC_REQUIRE(false, "cnn_backward: COMIC_OP_X3 is a bf16-plan layout");
      }
    } else if (op->kind <= 1) {
      const size_t dzb = dz_bytes_of(op, batch, sizeof(T));
      void* dz = st_w != st ? (void*)((char*)scratch + dz_off) : scratch;
      if (int rc = conv_backward<T>(op, buffers[op->src], xc, buffers[op->dst], gy, yc, gx, weights + op->weight,
                                    grads + op->weight, batch, dz, st_w != st ? (int64_t)dzb : scratch_bytes, st,
                                    filters_ready, st_w))
        return rc;
      dz_off += dzb;
    } else if (op->kind <= 4) {
      if (!gx) continue;
      if (int rc = pool_backward<T>(op, buffers[op->src], xc, gy, yc, gx, batch, st, x3 && op->kind <= 3)) return rc;
    } else {
      COMIC_REQUIRE(false, "cnn_backward: unknown op kind %d", op->kind);
    }
  }
  if (st_w != st) {      // join: what follows on st (all-reduce, optimiser) sees every weight gradient
    hipEvent_t ev;
    COMIC_REQUIRE(hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess, "cnn_backward: event");
    const bool ok = hipEventRecord(ev, st_w) == hipSuccess && hipStreamWaitEvent(st, ev, 0) == hipSuccess;
    (void)hipEventDestroy(ev);
    COMIC_REQUIRE(ok, "cnn_backward: join of the weight-gradient lane failed");
  }
  return 0;
}

// y += x; x = 0 (the join of the two chain lanes of comic_cnn_backward_sched)
template <typename T>
__global__ void add_clear_kernel(T* __restrict__ y, T* __restrict__ x, long n_chunks) {
  constexpr int EPC = Elem<T>::EPC;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_chunks) return;
  float a[EPC], b[EPC];
  load_vec<T>(y + i * EPC, a);
  load_vec<T>(x + i * EPC, b);
#pragma unroll
  for (int j = 0; j < EPC; ++j) {
    a[j] += b[j];
    b[j] = 0.f;
  }
  store_vec<T>(y + i * EPC, a);
  store_vec<T>(x + i * EPC, b);
}



template <typename T>
int cnn_backward_sched_impl(const comic_cnn_op* ops, int n_ops, const int32_t* sched, int n_sched, void* const* buffers,
                            void* const* grad_buffers, void* const* grad_alt, const int32_t* buf_channels,
                            const comic_conv_weight* weights, const comic_conv_grad* grads, int batch, void* scratch,
                            int64_t scratch_bytes, hipStream_t s0, hipStream_t s1, hipStream_t st_w, bool filters_ready,
                            bool no_act_fusion) {
  constexpr int EPC = Elem<T>::EPC;
  COMIC_REQUIRE(s1 && s1 != s0 && st_w && st_w != s0 && st_w != s1, "cnn_backward_sched: needs three distinct streams");
  COMIC_REQUIRE(backward_scratch_bytes(ops, n_ops, batch, sizeof(T), true) <= scratch_bytes,
                "cnn_backward_sched: scratch too small (every conv needs its own d-conv slice)");
  std::vector<size_t> dz_off((size_t)n_ops, 0), part_off((size_t)n_ops, 0);
  size_t off = 0;
  for (int i = 0; i < n_ops; ++i)
    if (ops[i].kind <= 1) {
      dz_off[i] = off;
      off += dz_bytes_of(ops + i, batch, sizeof(T));
    }
  const size_t part0 = off;
  for (int i = 0; i < n_ops; ++i)
    if (ops[i].kind <= 1) {
      part_off[i] = off;
      off += dbeta_partial_bytes(ops + i);
    }
  COMIC_REQUIRE(hipMemsetAsync((char*)scratch + part0, 0, off - part0, s0) == hipSuccess, "cnn_backward_sched: memset failed");
  // Activation-gradient fusion: conv p whose output slice is read by exactly one op, a conv i on the same lane, gets its d-conv
  // tensor and d beta from the epilogue of i's backward-data launch (the inner convs of the Inception branches: one launch
  // less per conv on the serial chain a block's longest branch is).  fused_by[p] = i, fuses[i] = p.
  std::vector<int> lane_of((size_t)n_ops, -1), fused_by((size_t)n_ops, -1), fuses((size_t)n_ops, -1);
  for (int k = 0; k < n_sched; ++k)
    if (sched[4 * k] == 0 && sched[4 * k + 1] >= 0 && sched[4 * k + 1] < n_ops) lane_of[sched[4 * k + 1]] = sched[4 * k + 2];
  if (!no_act_fusion)
    for (int i = 0; i < n_ops; ++i) {
      const comic_cnn_op& c = ops[i];
      if (c.kind != 0 || c.out_f32 || (c.flags & COMIC_OP_X3)) continue;
      int p = -1, readers = 0;
      for (int j = 0; j < n_ops; ++j) {
        const comic_cnn_op& o = ops[j];
        // every op that touches this channel range of the buffer as a source (pools, concats, convs)
        if (o.src == c.src && !(o.src_coff + o.Cin <= c.src_coff || c.src_coff + c.Cin <= o.src_coff)) ++readers;
        if (o.kind == 0 && o.dst == c.src && o.dst_coff == c.src_coff && o.Cout == c.Cin) p = j;
      }
      if (p < 0 || readers != 1) continue;
      const comic_cnn_op& q = ops[p];
      if (q.SH != 1 || q.SW != 1 || q.out_f32 || (q.flags & (COMIC_OP_X3 | COMIC_OP_RAW)) || lane_of[p] != lane_of[i] || lane_of[i] < 0) continue;
      // nothing else may write into that slice (a pool or a second conv) or read the gradient buffer's slice
      bool only_writer = true;
      for (int j = 0; j < n_ops; ++j)
        if (j != p && ops[j].dst == c.src && ops[j].kind != 5 && ops[j].kind != 6 &&
            !(ops[j].dst_coff + (ops[j].kind == 0 ? ops[j].Cout : ops[j].Cin) <= c.src_coff || c.src_coff + c.Cin <= ops[j].dst_coff))
          only_writer = false;
      if (!only_writer) continue;
      fused_by[p] = i;
      fuses[i] = p;
    }
  std::vector<char> seen((size_t)n_ops, 0);
  bool lane1_open = false;
  // Weight gradients of the convs inside a fork / join region (the branches of an Inception block) are launched at the
  // region's join, behind ONE fork of the weight-gradient lane, instead of one fork per conv between two launches of a
  // chain lane: an event record in front of every backward-data launch kept the chain lanes idle for longer than their
  // kernels ran (10-28 us between dependent launches of 6-25 us, profiles/r05_finetune_lanes.txt).  Every conv owns its
  // d-conv slice of the scratch, so a later launch reads the same bytes.  Outside the regions (the stem's serial chain of
  // large convs) a weight gradient still starts as soon as its d-conv tensor exists.
  std::vector<PendingWgrad> pend;
  auto flush_wgrads = [&]() -> int {
    if (pend.empty()) return 0;
    COMIC_REQUIRE(link_streams(s0, st_w), "cnn_backward_sched: fork of the weight-gradient lane failed");
    for (const PendingWgrad& w : pend)
      if (int rc = launch_wgrad<T>(w.op, w.x, w.xc, w.dz, w.gr, batch, st_w)) return rc;
    pend.clear();
    COMIC_LAUNCH_CHECK("cnn_backward_sched (weight gradients of a block)");
    return 0;
  };
  for (int k = 0; k < n_sched; ++k) {
    const int32_t* r = sched + 4 * k;
    if (r[0] == 1) {                       // FORK
      COMIC_REQUIRE(link_streams(s0, s1), "cnn_backward_sched: fork failed");
      lane1_open = true;
      continue;
    }
    if (r[0] == 2) {                       // JOIN_ADD
      COMIC_REQUIRE(link_streams(s1, s0), "cnn_backward_sched: join failed");
      lane1_open = false;
      if (int rc = flush_wgrads()) return rc;
      if (r[1] >= 0) {
        const comic_cnn_op* any = nullptr;
        for (int i = 0; i < n_ops && !any; ++i)
          if (ops[i].kind != 5 && ops[i].kind != 6 && ops[i].src == r[1]) any = ops + i;
        COMIC_REQUIRE(any && grad_buffers[r[1]] && grad_alt && grad_alt[r[1]], "cnn_backward_sched: no alternate buffer %d", r[1]);
        const long n = (long)batch * any->H * any->W * buf_channels[r[1]];
        COMIC_REQUIRE(n % EPC == 0, "cnn_backward_sched: buffer %d is not a whole number of 16-byte chunks", r[1]);
        if ((any->flags & COMIC_OP_X3) && any->kind <= 3 && any->kind != 1) {      // x3 plans: fp32 gradients of the logical channels
          COMIC_REQUIRE(n % 12 == 0, "cnn_backward_sched: buffer %d is not three regions of whole chunks", r[1]);
          hipLaunchKernelGGL((add_clear_kernel<float>), dim3((unsigned)cdiv64(n / 12, 256)), dim3(256), 0, s0,
                             (float*)grad_buffers[r[1]], (float*)grad_alt[r[1]], n / 12);
        } else
        hipLaunchKernelGGL((add_clear_kernel<T>), dim3((unsigned)cdiv64(n / EPC, 256)), dim3(256), 0, s0,
                           (T*)grad_buffers[r[1]], (T*)grad_alt[r[1]], n / EPC);
      }
      continue;
    }
    COMIC_REQUIRE(r[0] == 0 && r[1] >= 0 && r[1] < n_ops && !seen[r[1]], "cnn_backward_sched: bad schedule row %d", k);
    seen[r[1]] = 1;
    const comic_cnn_op* op = ops + r[1];
    COMIC_REQUIRE(r[2] == 0 || lane1_open, "cnn_backward_sched: lane 1 used outside a fork / join region");
    hipStream_t st = r[2] ? s1 : s0;
    void* gy = grad_buffers[op->dst];
    COMIC_REQUIRE(gy, "cnn_backward_sched: op %d has no output gradient buffer", r[1]);
    void* gx = r[3] ? (grad_alt ? grad_alt[op->src] : nullptr) : grad_buffers[op->src];
    COMIC_REQUIRE(!r[3] || gx, "cnn_backward_sched: op %d has no alternate input-gradient buffer", r[1]);
    const int xc = buf_channels[op->src], yc = buf_channels[op->dst];
    const bool x3 = (op->flags & COMIC_OP_X3) != 0;
    if (x3 && op->kind <= 1) {
      if constexpr (sizeof(T) == 2) {
        if (int rc = conv_backward_x3(op, buffers[op->src], xc, buffers[op->dst], (const float*)gy, yc, op->out_f32 ? yc : yc / 3,
                                      (float*)gx, op->kind == 1 ? 0 : xc / 3, weights + op->weight, grads + op->weight, batch,
                                      (char*)scratch + dz_off[r[1]], (int64_t)dz_bytes_of(op, batch, sizeof(T)), st, filters_ready, st_w))
          return rc;
      } else {
        COMIC_REQUIRE(false, "cnn_backward_sched: COMIC_OP_X3 is a bf16-plan layout");
      }
    } else if (op->kind <= 1) {
      void* dz = (char*)scratch + dz_off[r[1]];
      ConvMask mk{};
      const int p = fuses[r[1]];
      if (p >= 0) {
        COMIC_REQUIRE(!seen[p], "cnn_backward_sched: conv %d runs before its reader %d", p, r[1]);
        mk = ConvMask{buffers[ops[p].dst], buf_channels[ops[p].dst], ops[p].dst_coff, weights[ops[p].weight].scale,
                      (float*)((char*)scratch + part_off[p]), (char*)scratch + dz_off[p]};
        COMIC_REQUIRE(mk.y && mk.scale && grads[ops[p].weight].dbeta, "cnn_backward_sched: conv %d has no forward output / scale / d beta", p);
      }
      if (int rc = conv_backward<T>(op, buffers[op->src], xc, buffers[op->dst], gy, yc, gx, weights + op->weight,
                                    grads + op->weight, batch, dz, (int64_t)dz_bytes_of(op, batch, sizeof(T)), st,
                                    filters_ready, st_w, /*dz_ready=*/fused_by[r[1]] >= 0, p >= 0 ? &mk : nullptr,
                                    lane1_open ? &pend : nullptr))
        return rc;
    } else if (op->kind <= 4) {
      if (!gx) continue;
      if (int rc = pool_backward<T>(op, buffers[op->src], xc, gy, yc, gx, batch, st, x3 && op->kind <= 3)) return rc;
    } else {
      COMIC_REQUIRE(false, "cnn_backward_sched: unknown op kind %d", op->kind);
    }
  }
  COMIC_REQUIRE(!lane1_open, "cnn_backward_sched: the schedule ends inside a fork / join region");
  if (int rc = flush_wgrads()) return rc;
  for (int i = 0; i < n_ops; ++i)
    COMIC_REQUIRE(seen[i] || ops[i].kind == 5 || ops[i].kind == 6, "cnn_backward_sched: op %d is not in the schedule", i);
  {
    // the partial d beta rows of the fused convs -> d beta, on the weight-gradient lane (it waits for both chain lanes' launches
    // so far; the optimiser waits for this lane)
    DbetaFoldTable tb;
    tb.n = 0;
    auto flush = [&]() {
      if (tb.n) hipLaunchKernelGGL(dbeta_fold_kernel, dim3(tb.n), dim3(256), 0, st_w, tb);
      tb.n = 0;
    };
    bool any = false;
    for (int p = 0; p < n_ops; ++p) any = any || fused_by[p] >= 0;
    if (any) COMIC_REQUIRE(link_streams(s0, st_w), "cnn_backward_sched: fold of the fused d beta sums failed");
    for (int p = 0; p < n_ops; ++p) {
      if (fused_by[p] < 0) continue;
      if (tb.n == kFoldMax) flush();
      auto& en = tb.e[tb.n++];
      en.part = (const float*)((char*)scratch + part_off[p]);
      en.dbeta = grads[ops[p].weight].dbeta;
      en.C = ops[p].Cout;
      en.pad = 0;
    }
    flush();
  }
  COMIC_REQUIRE(link_streams(st_w, s0), "cnn_backward_sched: join of the weight-gradient lane failed");
  COMIC_LAUNCH_CHECK("cnn_backward_sched");
  return 0;
}

}  // namespace

extern "C" int comic_cnn_backward_sched(const comic_cnn_op* ops, int n_ops, const int32_t* sched, int n_sched,
                                        void* const* buffers, void* const* grad_buffers, void* const* grad_buffers_alt,
                                        const int32_t* buf_channels, const comic_conv_weight* weights,
                                        const comic_conv_grad* grads, int batch, int dtype, int filters_ready, void* scratch,
                                        int64_t scratch_bytes, void* stream0, void* stream1, void* wgrad_stream) {
  COMIC_REQUIRE(ops && sched && buffers && grad_buffers && buf_channels && weights && grads && scratch,
                "comic_cnn_backward_sched: null argument");
  COMIC_REQUIRE(dtype != COMIC_F16, "comic_cnn_backward_sched: f16 plans have no backward (cnn_finetune runs on bf16, bf16x3 or fp32 plans)");
  if (dtype == COMIC_BF16)
    return cnn_backward_sched_impl<bf16_t>(ops, n_ops, sched, n_sched, buffers, grad_buffers, grad_buffers_alt, buf_channels,
                                           weights, grads, batch, scratch, scratch_bytes, (hipStream_t)stream0,
                                           (hipStream_t)stream1, (hipStream_t)wgrad_stream, (filters_ready & 1) != 0,
                                          (filters_ready & COMIC_CNN_BWD_NO_ACT_FUSION) != 0);
  if (dtype == COMIC_F32)
    return cnn_backward_sched_impl<float>(ops, n_ops, sched, n_sched, buffers, grad_buffers, grad_buffers_alt, buf_channels,
                                          weights, grads, batch, scratch, scratch_bytes, (hipStream_t)stream0,
                                          (hipStream_t)stream1, (hipStream_t)wgrad_stream, (filters_ready & 1) != 0,
                                          (filters_ready & COMIC_CNN_BWD_NO_ACT_FUSION) != 0);
  COMIC_REQUIRE(false, "unknown dtype %d", dtype);
  return 2;
}


extern "C" int64_t comic_cnn_backward_scratch_bytes(const comic_cnn_op* ops, int n_ops, int batch, int dtype, int lanes) {
  if (!ops) return -1;
  if (dtype != COMIC_BF16 && dtype != COMIC_F32) {
    comic_set_error("comic_cnn_backward_scratch_bytes: dtype %d has no backward (bf16 or fp32 plans only)", dtype);
    return -1;
  }
  return backward_scratch_bytes(ops, n_ops, batch, dtype == COMIC_BF16 ? 2 : 4, lanes > 1);
}

extern "C" int comic_cnn_pack_x3_weights(const float* const* masters, void* const* outs, const int32_t* cout,
                                         const int32_t* taps, const int32_t* cin, int n, void* stream) {
  COMIC_REQUIRE(masters && outs && cout && taps && cin && n >= 0, "comic_cnn_pack_x3_weights: null argument");
  hipStream_t st = (hipStream_t)stream;
  PackX3Table tb;
  tb.n = 0;
  uint32_t blocks = 0;
  auto flush = [&]() {
    if (tb.n) hipLaunchKernelGGL(pack_x3_table_kernel, dim3(blocks), dim3(256), 0, st, tb);
    tb.n = 0;
    blocks = 0;
  };
  for (int i = 0; i < n; ++i) {
    COMIC_REQUIRE(masters[i] && outs[i] && cout[i] > 0 && cout[i] <= 65535 && cin[i] > 0 && cin[i] <= 65535 && taps[i] > 0 &&
                      taps[i] <= 65535, "comic_cnn_pack_x3_weights: bad entry %d", i);
    if (tb.n == kPackTableMax) flush();
    PackX3Entry& en = tb.e[tb.n++];
    en.master = masters[i];
    en.out = (bf16_t*)outs[i];
    en.first_block = blocks;
    en.cout = (uint16_t)cout[i]; en.cin = (uint16_t)cin[i]; en.taps = (uint16_t)taps[i]; en.pad = 0;
    const long K3 = 3L * taps[i] * cin[i];
    blocks += (uint32_t)cdiv64((long)cout[i] * ((K3 + 63) / 64 * 64), 256);
  }
  flush();
  COMIC_LAUNCH_CHECK("pack_x3_weights");
  return 0;
}

extern "C" int comic_cnn_pack_bwd_filters(const comic_cnn_op* ops, int n_ops, const comic_conv_grad* grads, int dtype,
                                          void* stream) {
  COMIC_REQUIRE(ops && grads, "comic_cnn_pack_bwd_filters: null argument");
  COMIC_REQUIRE(dtype != COMIC_F16, "comic_cnn_pack_bwd_filters: f16 plans have no backward (cnn_finetune runs on bf16, bf16x3 or fp32 plans)");
  if (dtype == COMIC_BF16) return pack_bwd_filters_impl<bf16_t>(ops, n_ops, grads, (hipStream_t)stream);
  if (dtype == COMIC_F32) return pack_bwd_filters_impl<float>(ops, n_ops, grads, (hipStream_t)stream);
  COMIC_REQUIRE(false, "unknown dtype %d", dtype);
  return 2;
}

extern "C" int comic_cnn_backward(const comic_cnn_op* ops, int n_ops, void* const* buffers, void* const* grad_buffers,
                                  const int32_t* buf_channels, const comic_conv_weight* weights,
                                  const comic_conv_grad* grads, int batch, int dtype, int filters_ready, void* scratch,
                                  int64_t scratch_bytes, void* stream, void* wgrad_stream) {
  COMIC_REQUIRE(ops && buffers && grad_buffers && buf_channels && weights && grads && scratch,
                "comic_cnn_backward: null argument");
  COMIC_REQUIRE(dtype != COMIC_F16, "comic_cnn_backward: f16 plans have no backward (cnn_finetune runs on bf16, bf16x3 or fp32 plans)");
  hipStream_t st = (hipStream_t)stream, st_w = (hipStream_t)wgrad_stream;
  if (dtype == COMIC_BF16)
    return cnn_backward_impl<bf16_t>(ops, n_ops, buffers, grad_buffers, buf_channels, weights, grads, batch, scratch,
                                     scratch_bytes, st, filters_ready != 0, st_w);
  if (dtype == COMIC_F32)
    return cnn_backward_impl<float>(ops, n_ops, buffers, grad_buffers, buf_channels, weights, grads, batch, scratch,
                                    scratch_bytes, st, filters_ready != 0, st_w);
  COMIC_REQUIRE(false, "unknown dtype %d", dtype);
  return 2;
}
