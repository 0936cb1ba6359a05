// Caption scoring: log p(target | image, prefix) for the R = T' * B teacher-forced rows of decoder outputs y, without the
// [R][V] logits ever reaching memory at a large vocabulary.
//
// Replaces, inside comic_decoder_score, the output projection + softmax cross-entropy of the teacher-forced graph
// (rnn_decoder_training, common/ops_rnn.py:183-243: logits = y W_o + b_o; _train_caption_model, src/model_base.py:325-347:
// sparse softmax cross-entropy weighted by the caption mask), keeping the per-token terms instead of the reduced loss.
//
// Large vocabulary (D % 128 == 0, V >= 4096: the conditions of the beam step's streaming projection):
//   * W_o in the packed hi / lo bf16 fragment layout of comic_beam_pack_wo (beam_pack.h: chunks of 112 columns, a chunk's
//     K-quarter = 56 contiguous KB) with its zero-padded bias, packed once per call; the same product arithmetic as
//     beam_logits.hip: hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16, D[v][row] orientation, a workgroup per chunk.
//   * Rows in blocks of 256 (eight waves x two 16-row tiles) as the FAST grid dimension, chunks as the slow one.  A chunk's
//     224 KB of fragments (D = 512) do not fit the 160 KB LDS beside anything else, so a loop over the row blocks inside the
//     workgroup would stream them again per block exactly as a second workgroup does: the re-stream bytes are the same
//     (52 MB x ceil(R / 256) at V = 25 599, from the L2 / MALL after the first block: the blocks of a chunk are dispatched
//     next to each other) and the grid form gives ceil(R / 256) x 229 workgroups to balance over 256 CUs instead of 229.
//     LDS: one 56 KB quarter + 448 B of bias, single-buffered (the next quarter's fragments and rows of y are requested
//     into registers before the barrier that frees the buffer); 155 VGPRs, i.e. one workgroup of eight waves per CU.
//   * y is read as fp32 and split into hi / lo in registers (8 floats per lane and k-step): no packed copy of y.
//   * per row and chunk the workgroup writes the chunk maximum, the chunk sum of exponentials (padded columns of the
//     ragged last chunk are -inf: they enter neither) and -- only the chunk that owns the target column -- the target's
//     logit: one writer per address, plain vector stores.
// Small vocabulary: the caller projects the rows with the GEMM into workspace; one wave per row does max / sum-exp / gather
// and writes the same three arrays with a single chunk.
// Merge (both): one thread per (t, b) combines the partials IN CHUNK ORDER, token_logp[t][b] = wmask * (logit - max - log sum)
// (exactly 0 where wmask == 0 or t >= lens[b]); a second launch sums each caption's tokens IN t ORDER.  No atomics and no
// reduction whose order depends on scheduling: the same bits in every run.
#include <float.h>

#include "beam_pack.h"
#include "common.h"

int comic_beam_pack_wo(const float* W_o, const float* b_o, int ld, void* wo_frag, int D, int V, hipStream_t st);
int comic_beam_logits_chunks(int V);
int64_t comic_beam_logits_pack_bytes(int D, int V);

namespace {

constexpr int kRowBlock = 256;          // rows per workgroup: 8 waves x 2 tiles of 16
constexpr int kScoreLds = kQuarterBytes + kChunkCols * 4;

struct ScoreArgs {
  const float* y;            // [R][D]
  const uint4* wo_frag;      // comic_beam_pack_wo
  const float* bias_pad;     // [chunks * kChunkCols]
  const int32_t* targets_bt; // [B][T]
  float* pmax;               // [chunks][R]
  float* psum;               // [chunks][R]
  float* tlogit;             // [R]
  int R, D, V, B, T;
};

__device__ __forceinline__ void split2(float a, float b, uint32_t& h, uint32_t& l) {
  h = pack_bf16x2(a, b);
  l = pack_bf16x2(a - __uint_as_float(h << 16), b - __uint_as_float(h & 0xFFFF0000u));
}
__device__ __forceinline__ void split8(const float4& a, const float4& b, bf16x8_t& hi, bf16x8_t& lo) {
  uint4 h, l;
  split2(a.x, a.y, h.x, l.x);
  split2(a.z, a.w, h.y, l.y);
  split2(b.x, b.y, h.z, l.z);
  split2(b.z, b.w, h.w, l.w);
  hi = __builtin_bit_cast(bf16x8_t, h);
  lo = __builtin_bit_cast(bf16x8_t, l);
}

// grid (row blocks, chunks), 512 threads
__global__ __launch_bounds__(512) void score_logits_kernel(ScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int rb = blockIdx.x, c = blockIdx.y;
  const int D = a.D, KS = D / 32, NQ = D / 128;
  const uint4* wsrc = (const uint4*)((const unsigned char*)a.wo_frag + (size_t)c * KS * kVT * 2 * 1024);
  uint4* wl = (uint4*)smem;
  float* bias_l = (float*)(smem + kQuarterBytes);
  if (tid < kChunkCols) bias_l[tid] = a.bias_pad[(size_t)c * kChunkCols + tid];

  int row[2];
  const float* yrow[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int r = rb * kRowBlock + (wave + 8 * m) * 16 + fr;
    row[m] = r < a.R ? r : -1;
    yrow[m] = a.y + (size_t)(r < a.R ? r : 0) * D + fg * 8;
  }
  f32x4_t acc[2][kVT];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int vt = 0; vt < kVT; ++vt) acc[m][vt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  constexpr int kQ16 = kQuarterBytes / 16;          // uint4 words of a quarter: kVT * 512
  for (int q = 0; q < NQ; ++q) {
    // the quarter's fragments and this wave's rows of y: requested together, the fragments go through registers to the LDS
    uint4 wreg[kVT];
#pragma unroll
    for (int i = 0; i < kVT; ++i) wreg[i] = wsrc[(size_t)q * kQ16 + i * 512 + tid];
    float4 yv[2][4][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float* src = yrow[m] + (q * 4 + s) * 32;
        yv[m][s][0] = *(const float4*)src;             // (rows past R read row 0: their columns of D are never stored)
        yv[m][s][1] = *(const float4*)(src + 4);
      }
    __syncthreads();                                  // the previous quarter is no longer read
#pragma unroll
    for (int i = 0; i < kVT; ++i) wl[i * 512 + tid] = wreg[i];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      bf16x8_t yh[2], yl[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) split8(yv[m][s][0], yv[m][s][1], yh[m], yl[m]);
#pragma unroll
      for (int vt = 0; vt < kVT; ++vt) {
        const bf16x8_t ah = __builtin_bit_cast(bf16x8_t, wl[((s * kVT + vt) * 2 + 0) * 64 + lane]);
        const bf16x8_t al = __builtin_bit_cast(bf16x8_t, wl[((s * kVT + vt) * 2 + 1) * 64 + lane]);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          acc[m][vt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, yh[m], acc[m][vt], 0, 0, 0);
          acc[m][vt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, yl[m], acc[m][vt], 0, 0, 0);
          acc[m][vt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, yh[m], acc[m][vt], 0, 0, 0);
        }
      }
    }
  }

  // lane (fr, fg) holds columns v = kChunkCols c + 16 vt + 4 fg + i (i < 4) of row row[m]
  const int v_base = c * kChunkCols + 4 * fg;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    int tgt = -1;
    if (row[m] >= 0) tgt = a.targets_bt[(size_t)(row[m] % a.B) * a.T + row[m] / a.B];
    float mx = -INFINITY, tl = 0.f;
    bool own = false;
#pragma unroll
    for (int vt = 0; vt < kVT; ++vt) {
      const float4 bb = *(const float4*)(bias_l + 16 * vt + 4 * fg);
      acc[m][vt][0] += bb.x; acc[m][vt][1] += bb.y; acc[m][vt][2] += bb.z; acc[m][vt][3] += bb.w;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int v = v_base + 16 * vt + i;
        if (v >= a.V) acc[m][vt][i] = -INFINITY;       // padded columns of the ragged last chunk: dead (exp -> 0)
        mx = fmaxf(mx, acc[m][vt][i]);
        if (v == tgt && v < a.V) {
          own = true;
          tl = acc[m][vt][i];
        }
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float se = 0.f;
#pragma unroll
    for (int vt = 0; vt < kVT; ++vt)
#pragma unroll
      for (int i = 0; i < 4; ++i) se += expf(acc[m][vt][i] - mx);
    // the four lane groups' partial sums: (s_r + s_r^16) + (s_r^32 + s_r^48), the same bits in all four lanes
    se += __shfl_xor(se, 16, 64);
    se += __shfl_xor(se, 32, 64);
    if (row[m] >= 0) {
      if (fg == 0) {
        a.pmax[(size_t)c * a.R + row[m]] = mx;
        a.psum[(size_t)c * a.R + row[m]] = se;
      }
      if (own) a.tlogit[row[m]] = tl;              // one lane of one chunk
    }
  }
}

// small vocabulary: one wave per row of the materialised logits [R][V]
__global__ __launch_bounds__(256) void score_rows_kernel(const float* __restrict__ logits, const int32_t* __restrict__ targets_bt,
                                                         float* __restrict__ pmax, float* __restrict__ psum,
                                                         float* __restrict__ tlogit, int R, int V, int B, int T) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const float* x = logits + (size_t)r * V;
  float mx = -INFINITY;
  for (int v = lane; v < V; v += 64) mx = fmaxf(mx, x[v]);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float se = 0.f;
  for (int v = lane; v < V; v += 64) se += expf(x[v] - mx);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) se += __shfl_xor(se, o, 64);     // butterfly: a fixed order, the same bits in every lane
  if (lane == 0) {
    const int tgt = targets_bt[(size_t)(r % B) * T + r / B];
    pmax[r] = mx;
    psum[r] = se;
    tlogit[r] = (tgt >= 0 && tgt < V) ? x[tgt] : 0.f;
  }
}

// token_logp[t][b] for every (t, b) of [T][B]; partials [chunks][R] are combined in chunk order
__global__ __launch_bounds__(256) void score_merge_kernel(const float* __restrict__ pmax, const float* __restrict__ psum,
                                                          const float* __restrict__ tlogit, const int32_t* __restrict__ targets_bt,
                                                          const float* __restrict__ wmask_bt, const int32_t* __restrict__ lens,
                                                          const unsigned* __restrict__ err, float* __restrict__ token_logp,
                                                          int chunks, int R, int B, int T, int V) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * B) return;
  const int t = i / B, b = i % B;
  const float w = wmask_bt[(size_t)b * T + t];
  const int tgt = targets_bt[(size_t)b * T + t];
  float out = 0.f;
  if (i < R && w != 0.f && t < lens[b] && tgt >= 0 && tgt < V) {
    float mx = -INFINITY;
    for (int c = 0; c < chunks; ++c) mx = fmaxf(mx, pmax[(size_t)c * R + i]);
    float se = 0.f;
    for (int c = 0; c < chunks; ++c) se += psum[(size_t)c * R + i] * expf(pmax[(size_t)c * R + i] - mx);
    out = w * ((tlogit[i] - mx) - logf(se));
  }
  if (err && err[0]) out = __uint_as_float(0x7fc00000u);      // a persistent loop of the forward timed out: no number
  token_logp[i] = out;
}

// caption_logp[b] = sum over t, in t order
__global__ __launch_bounds__(256) void score_caption_kernel(const float* __restrict__ token_logp, float* __restrict__ caption_logp,
                                                            int B, int T) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float s = 0.f;
  for (int t = 0; t < T; ++t) s += token_logp[(size_t)t * B + b];
  caption_logp[b] = s;
}

}  // namespace

bool comic_score_stream_supported(int D, int V) { return D % 128 == 0 && D >= 128 && D <= 1024 && V >= 4096; }

// scratch of the projection for `rows` rows: packed W_o + partials on the streaming path, logits + partials otherwise
int64_t comic_score_logits_ws_bytes(int D, int V, long rows, int stream) {
  auto up = [](int64_t n) { return (n + 255) & ~(int64_t)255; };
  if (stream) return up(comic_beam_logits_pack_bytes(D, V)) + 2 * up(4ll * comic_beam_logits_chunks(V) * rows) + up(4ll * rows);
  return up(4ll * rows * V) + 3 * up(4ll * rows);
}
float* comic_score_logits_buffer(void* ws) { return (float*)ws; }      // small path: where the caller's GEMM writes [R][V]

// y [Tp * B][D] (streaming) or the logits the caller wrote into comic_score_logits_buffer(ws) -> token_logp [T][B], caption_logp [B]
int comic_score_logits(const float* y, const float* W_o, const float* b_o, const int32_t* targets_bt, const float* wmask_bt,
                       const int32_t* lens, const unsigned* err, int B, int T, int Tp, int D, int V, int stream,
                       float* token_logp_tb, float* caption_logp, void* ws, int64_t ws_bytes, hipStream_t st) {
  const int R = Tp * B;
  COMIC_REQUIRE(ws && ws_bytes >= comic_score_logits_ws_bytes(D, V, R, stream), "score_logits: workspace too small");
  auto up = [](int64_t n) { return (n + 255) & ~(int64_t)255; };
  char* base = (char*)ws;
  float *pmax, *psum, *tl;
  int chunks = 1;
  if (stream) {
    COMIC_REQUIRE(comic_score_stream_supported(D, V), "score_logits: unsupported shape (D %d, V %d)", D, V);
    chunks = comic_beam_logits_chunks(V);
    void* wo_frag = base;
    base += up(comic_beam_logits_pack_bytes(D, V));
    pmax = (float*)base; base += up(4ll * chunks * R);
    psum = (float*)base; base += up(4ll * chunks * R);
    tl = (float*)base;
    if (comic_beam_pack_wo(W_o, b_o, V, wo_frag, D, V, st)) return 1;
    ScoreArgs a{};
    a.y = y; a.wo_frag = (const uint4*)wo_frag;
    a.bias_pad = (const float*)((const uint4*)wo_frag + (size_t)chunks * (D / 32) * kVT * 2 * 64);
    a.targets_bt = targets_bt; a.pmax = pmax; a.psum = psum; a.tlogit = tl;
    a.R = R; a.D = D; a.V = V; a.B = B; a.T = T;
    static PerDeviceOnce once;
    if (!once.slot()) {
      COMIC_REQUIRE(hipFuncSetAttribute((const void*)score_logits_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        kScoreLds) == hipSuccess, "score_logits: cannot raise the LDS limit");
      once.slot() = true;
    }
    hipLaunchKernelGGL(score_logits_kernel, dim3((R + kRowBlock - 1) / kRowBlock, chunks), dim3(512), kScoreLds, st, a);
    COMIC_LAUNCH_CHECK("score_logits");
  } else {
    const float* logits = (const float*)base;
    base += up(4ll * R * V);
    pmax = (float*)base; base += up(4ll * R);
    psum = (float*)base; base += up(4ll * R);
    tl = (float*)base;
    hipLaunchKernelGGL(score_rows_kernel, dim3((R + 3) / 4), dim3(256), 0, st, logits, targets_bt, pmax, psum, tl, R, V, B, T);
    COMIC_LAUNCH_CHECK("score_rows");
  }
  hipLaunchKernelGGL(score_merge_kernel, dim3((unsigned)cdiv64((int64_t)T * B, 256)), dim3(256), 0, st, pmax, psum, tl, targets_bt,
                     wmask_bt, lens, err, token_logp_tb, chunks, R, B, T, V);
  COMIC_LAUNCH_CHECK("score_merge");
  hipLaunchKernelGGL(score_caption_kernel, dim3((B + 255) / 256), dim3(256), 0, st, token_logp_tb, caption_logp, B, T);
  COMIC_LAUNCH_CHECK("score_caption");
  return 0;
}
