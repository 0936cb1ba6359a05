// Native executors for the attention-LSTM decoder: one teacher-forced forward+backward
// (XE or SCST-weighted), greedy decode and beam search.  They issue the step kernels of
// decoder.hip / gemm.hip / decode.hip on one HIP stream with no host synchronisation and no
// allocation (caller-provided workspace), so a whole step can be captured in a hipGraph.
//
// Mirrors (not translates) the reference graph builders:
//   ModelBase._decoder_rnn / _decoder_rnn_scst ...... src/model_base.py:109-269
//   rnn_decoder_training / _search / _beam_search ... common/ops_rnn.py:49-243
//   MultiHeadAttentionWrapperV3.call ................ common/ops_rnn.py:660-755
//   _train_caption_model (losses) ................... src/model_base.py:325-405
// Differences by design: the x-independent pieces are hoisted out of the time loop
// (embedding lookup for all steps, output projection + cross-entropy as one batched GEMM,
// all weight-gradient GEMMs batched over time), states are kept per step for the backward
// pass instead of TF's TensorArray stack, and dropout masks are explicit inputs.
#include <atomic>
#include <stdlib.h>

#include <algorithm>
#include <string.h>

#include "common.h"
#include "decoder_math.h"
#include "decoder_persist.h"
#include "exec_entries.h"
#include "gemm_group.h"
#include "lstm_prep.h"
#include "lstm_stream_dev.h"

// internal cross-file entries (gemm.hip, decoder.hip); the executor-only forms of the step kernels: exec_entries.h
int comic_gemm_f32_ws(const float* A, const float* B, float* C, const float* bias, int M, int N, int K, int lda,
                      int ldb, int ldc, int trans_a, int trans_b, float alpha, float beta, void* ws, int64_t ws_bytes,
                      hipStream_t st);
int comic_embed_bwd_set(const int32_t* ids, const float* dout, float* dtable, int rows, int E, int V, hipStream_t st);
// gemm.hip
int comic_gemm_bf16x3_impl(const float* A, const float* B, float* C, const float* bias, int M, int N, int K, int lda,
                           int ldb, int ldc, int trans_a, int trans_b, float alpha, float beta, void* ws,
                           int64_t ws_bytes, hipStream_t st);
// score_logits.hip
bool comic_score_stream_supported(int D, int V);
int64_t comic_score_logits_ws_bytes(int D, int V, long rows, int stream);
float* comic_score_logits_buffer(void* ws);
int comic_score_logits(const float* y, const float* W_o, const float* b_o, const int32_t* targets_bt, const float* wmask_bt,
                       const int32_t* lens, const unsigned* err, int B, int T, int Tp, int D, int V, int stream,
                       float* token_logp_tb, float* caption_logp, void* ws, int64_t ws_bytes, hipStream_t st);
// beam_step.hip
int comic_beam_step_ws(const float* logits, float* log_probs, int32_t* finished, int64_t* lengths, int32_t* word_ids,
                       int32_t* parent_ids, float* scores, int B, int W, int V, int end_id, float lpw, void* ws,
                       int64_t ws_bytes, hipStream_t st);
int64_t comic_beam_step_split_bytes(int n, int B, int W, int chunks);
int comic_beam_groups_check(const comic_beam_groups* g, const char* who, int W, int V);
int comic_beam_sampling_check(const comic_beam_sampling* s, const char* who, float lpw, int W);
int64_t comic_beam_step_required_bytes(int n, int B, int W, int chunks);
// beam_truncate.hip
int comic_beam_truncation_check(const comic_beam_truncation* tr, const char* who, int V, bool whole);
// beam_bans.hip
int comic_beam_constraints_check(const comic_beam_constraints* c, const char* who, int W, int V, int end_id, int max_steps,
                                 bool whole);
int comic_beam_bans_launch(const int32_t* prev_words, const int32_t* prev_parents, const int32_t* finished,
                           const int64_t* lengths, int32_t* hist, uint32_t* bits, int t, int B, int W, int V, int max_steps,
                           int end_id, const comic_beam_constraints* c, hipStream_t st);
// beam_required.hip
int comic_beam_required_check(const comic_beam_required* q, const char* who, int W, int V, int end_id, int max_steps,
                              const comic_beam_constraints* cons);
int comic_beam_required_launch(const int32_t* prev_words, const int32_t* prev_parents, const int32_t* req, int32_t* hist,
                               int32_t* base, int32_t* special, const comic_beam_required* q, int t, int B, int W, int V,
                               int max_steps, int write_hist, hipStream_t st);
int comic_beam_required_init_launch(const int32_t* req, float* log_probs, int32_t* finished, int64_t* lengths, int B, int W,
                                    const comic_beam_required* q, hipStream_t st);
// beam_prefix.hip
int comic_beam_prefix_check(const comic_beam_prefix* p, const char* who, int V, int max_steps);
int comic_beam_prefix_launch(const int32_t* pfx, const int32_t* finished, uint32_t* bits, int t, int B, int W, int V, int P,
                             int has_bans, hipStream_t st);
// decode.hip
int comic_ens_gather_state(const float* c, const float* h, const float* att, const int32_t* parent, float* c_out,
                           float* h_out, float* att_out, int R, int W, int D, int A, hipStream_t st);

namespace {

// Executor switches come with the call (comic_decoder_desc::flags, COMIC_DEC_*): the library reads no environment.
// The entry points latch them for the calling thread; the helpers below are what the executors consult.
thread_local uint32_t g_dec_flags = 0;
struct FlagScope {
  explicit FlagScope(const comic_decoder_desc* d) {
    g_dec_flags = d ? d->flags : 0u;
    // LN_LSTM / GRU run on the per-step launch chain: the fused / streaming / persistent kernels are BasicLSTMCell's
    if (d && d->cell != COMIC_CELL_LSTM) g_dec_flags |= COMIC_DEC_NO_FUSED_STEP | COMIC_DEC_NO_PERSIST | COMIC_DEC_NO_PERSIST_BWD;
    comic_persist_set_stamps((g_dec_flags & COMIC_DEC_STAMPS) != 0);
  }
  ~FlagScope() { comic_persist_set_stamps(false); }
};
bool split_attn_bwd_enabled() { return !(g_dec_flags & COMIC_DEC_NO_SPLIT_ATTN_BWD); }
bool fused_step_enabled() { return !(g_dec_flags & COMIC_DEC_NO_FUSED_STEP); }
bool persist_enabled() { return !(g_dec_flags & COMIC_DEC_NO_PERSIST); }
bool persist_bwd_enabled() { return !(g_dec_flags & COMIC_DEC_NO_PERSIST_BWD); }
bool beam_logits_enabled() { return !(g_dec_flags & COMIC_DEC_NO_BEAM_LOGITS); }
bool lstm_stream_enabled() { return !(g_dec_flags & COMIC_DEC_NO_LSTM_STREAM); }
bool group_gemm_enabled() { return !(g_dec_flags & (COMIC_DEC_NO_GROUP_GEMM | COMIC_DEC_EXACT_GEMM)); }

// A second stream inside the training executor: the weight-gradient products after the backward loop are independent
// chains of mid-sized GEMMs and small reductions; two lanes fill each other's tails and launch gaps
// (COMIC_DEC_ONE_LANE: one stream).  Fork / join with events, so a hipGraph capture of the step takes both lanes.
struct SideLane {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
};
SideLane* side_lane() {
  static SideLane lanes[64];
  if (g_dec_flags & COMIC_DEC_ONE_LANE) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  SideLane* L = &lanes[dev];
  if (!L->s) {
    if (hipStreamCreateWithFlags(&L->s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&L->fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&L->join, hipEventDisableTiming) != hipSuccess) {
      L->s = nullptr;
      return nullptr;
    }
  }
  return L;
}

thread_local void* g_splitk_ws = nullptr;   // split-K scratch of the GEMM helpers below (one per lane)

// Fork / join of the side lane as a scope: whatever path leaves the scope (every RC(...) can return early), the lane
// is joined back into the caller's stream and the split-K scratch pointer is restored -- a capture of the step is
// never left with an unjoined stream, and a later step is never ordered behind the stragglers of a failed one.
struct LaneScope {
  SideLane* L;
  hipStream_t st;
  void* saved_ws;
  bool forked = false;
  int rc = 0;
  LaneScope(SideLane* lane, hipStream_t main, void* lane_ws) : L(lane), st(main), saved_ws(g_splitk_ws) {
    if (!L) return;
    if (hipEventRecord(L->fork, st) != hipSuccess || hipStreamWaitEvent(L->s, L->fork, 0) != hipSuccess) {
      comic_set_error("train_step: cannot fork the side lane");
      rc = 2;
      return;
    }
    forked = true;
    g_splitk_ws = lane_ws;
  }
  hipStream_t lane() const { return forked ? L->s : st; }
  void main_ws() { g_splitk_ws = saved_ws; }      // launches on the caller's stream from here on
  int join() {
    g_splitk_ws = saved_ws;
    if (!forked) return 0;
    forked = false;
    if (hipEventRecord(L->join, L->s) != hipSuccess || hipStreamWaitEvent(st, L->join, 0) != hipSuccess) {
      comic_set_error("train_step: cannot join the side lane");
      return 2;
    }
    return 0;
  }
  ~LaneScope() { (void)join(); }
};

#define RC(x)               \
  do {                      \
    int rc__ = (x);         \
    if (rc__) return rc__;  \
  } while (0)

struct Bump {
  char* base;
  size_t off, cap;
  bool ok;
  Bump(void* p, size_t c) : base((char*)p), off(0), cap(c), ok(true) {}
  template <typename T>
  T* take(size_t n) {
    const size_t bytes = (n * sizeof(T) + 255) & ~(size_t)255;
    if (base && off + bytes > cap) ok = false;
    T* r = base ? (T*)(base + off) : nullptr;
    off += bytes;
    return r;
  }
};

// xh_row = [ drop(x) ; drop(att) ; h ]   (cell_input_fn concat + DropoutWrapper input dropout)
__global__ void assemble_input_kernel(const float* __restrict__ x, const float* __restrict__ att,
                                      const float* __restrict__ h, const float* __restrict__ mask, float keep,
                                      float* __restrict__ xh, int B, int E, int A, int D) {
  const int W = E + A + D;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * W) return;
  const int b = i / W, c = i % W;
  float v;
  if (c < E + A) {
    v = c < E ? x[(size_t)b * E + c] : att[(size_t)b * A + (c - E)];
    if (mask) v = (v / keep) * mask[(size_t)b * (E + A) + c];
  } else {
    v = h ? h[(size_t)b * D + (c - E - A)] : 0.f;
  }
  xh[i] = v;
}

// xh_all[t][b][0:E] = drop(emb[ids[t,b]]) for every step at once (embedding lookup hoisted out
// of the time loop; the attention / recurrent parts of the row are filled by the step kernels)
__global__ void embed_to_xh_kernel(const float* __restrict__ table, const int32_t* __restrict__ ids_tb,
                                   const float* __restrict__ mask, float keep, float* __restrict__ xh, long rows,
                                   int E, int V, int EA, int Wd) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * E) return;
  const long r = i / E;
  const int e = (int)(i % E);
  const int id = ids_tb[r];
  float v = (id >= 0 && id < V) ? table[(size_t)id * E + e] : 0.f;
  if (mask) v = (v / keep) * mask[(size_t)r * EA + e];
  xh[(size_t)r * Wd + e] = v;
}

// The operand rows before the time loop, one launch: x parts of EVERY step (embedding lookup + input dropout, ids read
// from the batch-major table and also written time-major for the embedding backward), and step 0's att part (zero;
// att_all[0] too) and h part (h0).
__global__ void embed_step0_kernel(const float* __restrict__ table, const int32_t* __restrict__ ids_bt,
                                   int32_t* __restrict__ ids_tb, const float* __restrict__ mask, float keep,
                                   float* __restrict__ xh, float* __restrict__ att0, const float* __restrict__ h0, int Tp,
                                   int B, int T, int E, int A, int D, int V, float* __restrict__ xh_init,
                                   const float* __restrict__ cell_g, float* __restrict__ cell_gates,
                                   float* __restrict__ cell_cnew, float* __restrict__ c0, float* __restrict__ h0_out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n_x = (long)Tp * B * E;
  const int EA = E + A, Wd = E + A + D;
  if (i < n_x) {
    const long r = i / E;
    const int e = (int)(i % E), t = (int)(r / B), b = (int)(r % B);
    const int id = ids_bt[(size_t)b * T + t];
    if (e == 0) ids_tb[r] = id;
    float v = (id >= 0 && id < V) ? table[(size_t)id * E + e] : 0.f;
    if (mask) v = (v / keep) * mask[(size_t)r * EA + e];
    xh[(size_t)r * Wd + e] = v;
  } else if (i < n_x + (long)B * A) {
    const long j = i - n_x;
    att0[j] = 0.f;
    xh[(size_t)(j / A) * Wd + E + (j % A)] = 0.f;
  } else if (i < n_x + (long)B * A + (long)B * D) {
    const long j = i - n_x - (long)B * A;
    float hv;
    if (cell_g) {      // the rnn-init step's LSTM cell from a zero state (lstm_gates_fwd_kernel's arithmetic; the bias is in g)
      const int b = (int)(j / D), dd = (int)(j % D);
      const float* gr = cell_g + (size_t)b * 4 * D;
      const float si = sigmoidf_(gr[dd]), tj = tanhf(gr[D + dd]);
      const float sf = sigmoidf_(gr[2 * D + dd] + 1.0f), so = sigmoidf_(gr[3 * D + dd]);
      const float c2 = 0.f * sf + si * tj;
      hv = tanhf(c2) * so;
      float* ga = cell_gates + (size_t)b * 4 * D;
      ga[dd] = si; ga[D + dd] = tj; ga[2 * D + dd] = sf; ga[3 * D + dd] = so;
      cell_cnew[j] = c2;
      c0[j] = c2;
      h0_out[j] = hv;
    } else {
      hv = h0[j];
    }
    xh[(size_t)(j / D) * Wd + EA + (j % D)] = hv;
  } else if (xh_init && i < n_x + (long)B * A + 2L * B * D) {   // zero state of the init step: the h third of its operand rows
    const long j = i - n_x - (long)B * A - (long)B * D;
    xh_init[(size_t)(j / D) * Wd + EA + (j % D)] = 0.f;
  }
}

// inference step operand: xh[r] = [ emb[ids[r]] ; att[src(r)] ; h[src(r)] ], c_in[r] = c[src(r)] with
// src(r) = the beam-search parent of row r in the previous step (identity for greedy / step 0): the
// embedding lookup, the three state gathers and the concat of one step in a single pass.
__global__ void infer_prep_kernel(const float* __restrict__ table, const int32_t* __restrict__ ids,
                                  const int32_t* __restrict__ parent, int W, const float* __restrict__ att,
                                  const float* __restrict__ h, const float* __restrict__ c, float* __restrict__ xh,
                                  float* __restrict__ c_in, int R, int E, int A, int D, int V,
                                  const int32_t* __restrict__ stop, int stop_t) {
  // after the loop has ended the previous step's ids / parents were never written: nothing to gather
  if (comic_stopped(stop, stop_t)) return;
  const int Wd = E + A + D, cols = Wd + D;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)R * cols) return;
  const int r = (int)(i / cols), k = (int)(i % cols);
  const int src = parent ? (r / W) * W + min(max(parent[r], 0), W - 1) : r;
  if (k < E) {
    const int id = ids[r];
    xh[(size_t)r * Wd + k] = (id >= 0 && id < V) ? table[(size_t)id * E + k] : 0.f;
  } else if (k < E + A) {
    xh[(size_t)r * Wd + k] = att[(size_t)src * A + (k - E)];
  } else if (k < Wd) {
    xh[(size_t)r * Wd + k] = h[(size_t)src * D + (k - E - A)];
  } else {
    c_in[(size_t)r * D + (k - Wd)] = c[(size_t)src * D + (k - Wd)];
  }
}

// context-layer path only: att_next = fin ? att_prev : att_cur ; xh_next[:, E:E+A] = drop(att_next)
__global__ void select_att_kernel(const float* __restrict__ prev, const float* __restrict__ cur,
                                  const int32_t* __restrict__ lens, int t, float* __restrict__ dst,
                                  float* __restrict__ xh_next, int xh_ld, const float* __restrict__ mask_next,
                                  int mask_ld, float keep, int B, int A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * A) return;
  const int b = i / A, c = i % A;
  const float v = (lens && t >= lens[b]) ? prev[i] : cur[i];
  dst[i] = v;
  if (xh_next) {
    float x = v;
    if (mask_next) x = (x / keep) * mask_next[(size_t)b * mask_ld + c];
    xh_next[(size_t)b * xh_ld + c] = x;
  }
}

// dst = fin ? prev : cur      (impute_finished state select; lens NULL -> copy cur)
__global__ void select_rows_kernel(const float* __restrict__ prev, const float* __restrict__ cur,
                                   const int32_t* __restrict__ lens, int t, float* __restrict__ dst, int B, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C;
  dst[i] = (lens && t >= lens[b]) ? prev[i] : cur[i];
}

// live = !(t >= lens[b]):  out_live = d*live ; d = d*(1-live)
__global__ void split_live_kernel(float* __restrict__ d, float* __restrict__ out_live,
                                  const int32_t* __restrict__ lens, int t, int B, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C;
  const bool fin = lens && t >= lens[b];
  const float v = d[i];
  out_live[i] = fin ? 0.f : v;
  d[i] = fin ? v : 0.f;
}

// dxh [B, E+A+D] -> demb_t [B,E] = drop'(dxh[:, :E]); datt += drop'(dxh[:, E:E+A]); dh += dxh[:, E+A:]
// `carry`: datt holds d(att state after this step); only FINISHED rows carry it through to the
// state before the step (live rows' share went into the context inside attn_bwd).
__global__ void input_bwd_kernel(const float* __restrict__ dxh, const float* __restrict__ mask, float keep,
                                 float* __restrict__ demb, float* __restrict__ datt, float* __restrict__ dh,
                                 const int32_t* __restrict__ lens, int t, int carry, int B, int E, int A, int D,
                                 int S) {
  const int W = E + A + D;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * W) return;
  const int b = i / W, c = i % W;
  float v = dxh[i];
  for (int s = 1; s < S; ++s) v += dxh[(size_t)s * B * W + i];  // split-K partials of dg * K^T
  if (c < E + A) {
    if (mask) v = (v / keep) * mask[(size_t)b * (E + A) + c];
    if (c < E) {
      if (demb) demb[(size_t)b * E + c] = v;
    } else {
      float* p = datt + (size_t)b * A + (c - E);
      const bool fin = lens && t >= lens[b];
      *p = ((carry && !fin) ? 0.f : *p) + v;
    }
  } else {
    dh[(size_t)b * D + (c - E - A)] += v;
  }
}

// flat[b,t,m] = sum_h hist[t,b,h,m];  map_loss = mean((1-flat)^2)*scale;
// dmap[t,b,m] = 2*(flat-1)/(B*Tp*M)*scale.   Single workgroup (deterministic).
// two stages (fixed partition -> deterministic): per-workgroup partial sums, then one workgroup
__global__ __launch_bounds__(256) void maploss_part_kernel(const float* __restrict__ hist, float* __restrict__ dmap,
                                                           float* __restrict__ partial, int Tp, int B, int H, int M,
                                                           float scale) {
  __shared__ float red[256];
  const long n = (long)Tp * B * M;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  float acc = 0.f;
  if (i < n) {
    const int m = (int)(i % M);
    const long tb = i / M;
    const float* p = hist + (size_t)tb * H * M + m;
    float f = 0.f;
    for (int h = 0; h < H; ++h) f += p[(size_t)h * M];
    const float d = 1.0f - f;
    acc = d * d;
    if (dmap) dmap[i] = 2.0f * (f - 1.0f) / (float)n * scale;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
// the four attention-parameter gradients out of the column-summed [v | ln_g | ln_b | tau] row
__global__ void scatter_pgrad_kernel(const float* __restrict__ row, float* __restrict__ v, float* __restrict__ ln_g,
                                     float* __restrict__ ln_b, float* __restrict__ tau, int D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < D) {
    v[i] = row[i];
    ln_g[i] = row[D + i];
    ln_b[i] = row[2 * D + i];
  }
  if (i == 0) tau[0] = row[3 * D];
}

__global__ __launch_bounds__(256) void maploss_final_kernel(const float* __restrict__ partial, int nparts, long n,
                                                            float scale, float* __restrict__ map_loss) {
  __shared__ float red[256];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) acc += partial[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) map_loss[0] = red[0] / (float)n * scale;
}

__global__ __launch_bounds__(1024) void maploss_kernel(const float* __restrict__ hist, float* __restrict__ dmap,
                                                       float* __restrict__ map_loss, int Tp, int B, int H, int M,
                                                       float scale) {
  __shared__ float red[1024];
  const long n = (long)Tp * B * M;
  float acc = 0.f;
  for (long i = threadIdx.x; i < n; i += 1024) {
    const int m = (int)(i % M);
    const long tb = i / M;
    const float* p = hist + (size_t)tb * H * M + m;
    float f = 0.f;
    for (int h = 0; h < H; ++h) f += p[(size_t)h * M];
    const float d = 1.0f - f;
    acc += d * d;
    if (dmap) dmap[i] = 2.0f * (f - 1.0f) / (float)n * scale;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0 && map_loss) map_loss[0] = red[0] / (float)n * scale;
}

__global__ void fill_kernel(float* p, float v, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
__global__ void fill_i32_kernel(int32_t* p, int32_t v, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
// transpose int32 [B,T] -> [T,B] (first Tp rows)
__global__ void transpose_ids_kernel(const int32_t* __restrict__ in_bt, int32_t* __restrict__ out_tb, int B, int T,
                                     int Tp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Tp * B) return;
  const int t = i / B, b = i % B;
  out_tb[i] = in_bt[(size_t)b * T + t];
}
// tile_batch: out[b*W + w, :] = in[b, :]
__global__ void tile_rows_kernel(const float* __restrict__ in, float* __restrict__ out, long total, int W, int cols) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long r = i / cols;
  out[i] = in[(size_t)(r / W) * cols + (i % cols)];
}
// greedy bookkeeping: first_eos[b] = min(first_eos[b], t) when ids[b] == end,
// in one workgroup, plus the loop end -- steps_done = t+1 at the first step after which
// every row has emitted EOS (dynamic_decode stops there; later steps' kernels return at once, see ComicStop)
__global__ void eos_track_done_kernel(const int32_t* __restrict__ ids, int32_t* __restrict__ first_eos, int t,
                                      int end_id, int B, int32_t* __restrict__ steps_done, int max_steps) {
  __shared__ int any_live;
  if (threadIdx.x == 0) any_live = 0;
  __syncthreads();
  if (steps_done[0] <= t) return;                 // loop already over: ids of this step were never produced
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    int fe = first_eos[b];
    if (ids[b] == end_id && fe > t) {
      fe = t;
      first_eos[b] = t;
    }
    if (fe > t) any_live = 1;
  }
  __syncthreads();
  if (threadIdx.x == 0 && !any_live && steps_done[0] == max_steps) steps_done[0] = t + 1;
}
// beam bookkeeping: steps_executed = t+1 at the first step after which every beam is finished
__global__ void all_finished_kernel(const int32_t* __restrict__ finished, int32_t* __restrict__ steps_executed, int t,
                                    int n, int max_steps) {
  __shared__ int any_live;
  if (threadIdx.x == 0) any_live = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x)
    if (!finished[i]) any_live = 1;
  __syncthreads();
  if (threadIdx.x == 0 && !any_live && steps_executed[0] == max_steps) steps_executed[0] = t + 1;
}

__global__ void beam_init_kernel(float* __restrict__ log_probs, int32_t* __restrict__ finished,
                                 int64_t* __restrict__ lengths, int R, int W) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R) return;
  const bool first = (i % W) == 0;
  log_probs[i] = first ? 0.f : -INFINITY;
  finished[i] = first ? 0 : 1;
  lengths[i] = 0;
}

// out[r][c] = in[r][c] for c < cols, 0 in the padding columns (rows of `ld` >= cols elements)
__global__ void pad_rows_kernel(const float* __restrict__ in, float* __restrict__ out, int cols, int ld, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long r = i / ld;
  const int c = (int)(i - r * ld);
  out[i] = c < cols ? in[r * cols + c] : 0.f;
}

inline int fill(float* p, float v, long n, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(fill_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, p, v, n);
  COMIC_LAUNCH_CHECK("fill");
  return 0;
}
// split-K scratch of the running executor call (carved from the caller's workspace)
constexpr int64_t kSplitKBytes = 32ll << 20;

inline int gemm(const float* A, const float* B, float* C, const float* bias, int M, int N, int K, int lda, int ldb,
                int ldc, int ta, int tb, float beta, hipStream_t st) {
  return comic_gemm_f32_ws(A, B, C, bias, M, N, K, lda, ldb, ldc, ta, tb, 1.0f, beta, g_splitk_ws,
                           g_splitk_ws ? kSplitKBytes : 0, st);
}

// The time-batched products (hundreds of rows: keys, logits, d logits * W_o^T, every weight gradient) go
// to the bf16 matrix cores with hi/lo-split operands (comic_gemm_f32_split3, product error ~2^-15); the
// per-step products keep exact fp32 MFMAs.  COMIC_DEC_EXACT_GEMM selects the exact kernels everywhere.
inline int gemm_big(const float* A, const float* B, float* C, const float* bias, int M, int N, int K, int lda, int ldb,
                    int ldc, int ta, int tb, float beta, hipStream_t st) {
  const bool on = !(g_dec_flags & COMIC_DEC_EXACT_GEMM);
  if (!on || (long)M * N < 64 * 256 || K < 64)
    return gemm(A, B, C, bias, M, N, K, lda, ldb, ldc, ta, tb, beta, st);
  return comic_gemm_bf16x3_impl(A, B, C, bias, M, N, K, lda, ldb, ldc, ta, tb, 1.0f, beta, g_splitk_ws,
                                g_splitk_ws ? kSplitKBytes : 0, st);
}

// The products of a training step that do not feed the recurrence, as ONE grouped launch (gemm_group.hip): problems are
// collected here and run together; `slab` / `tickets` come from the step's workspace (kGroupTickets counters, zeroed at
// the top of the step and left zero by every launch).
constexpr int kGroupTickets = 4096;
struct GemmGroupRun {
  ComicGemmGroup g{};
  ComicGemmProb* add(int type, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc) {
    if (g.n >= kGemmGroupMax) return nullptr;
    ComicGemmProb& p = g.p[g.n++];
    p = ComicGemmProb{};
    p.type = type; p.A = A; p.B = B; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.alpha = 1.f; p.beta = 0.f; p.keep = 1.f;
    return &p;
  }
  // column sums of B [K][N] (ldb) -> C [N]
  ComicGemmProb* add_colsum(const float* B, float* C, int N, int K, int ldb) {
    ComicGemmProb* p = add(COMIC_GG_TN, nullptr, B, C, 1, N, K, 1, ldb, N);
    if (p) p->ones_a = 1;
    return p;
  }
  int run(void* slab, int64_t slab_cap, unsigned* tickets, hipStream_t st) {
    if (g.n == 0) return 0;
    int target = kGemmGroupTargetItems;
    for (;;) {
      int64_t need = 0;
      int nt = 0;
      const int wg = comic_gemm_group_plan(g, target, &need, &nt);
      if (wg < 0) return 2;
      if (need <= slab_cap && nt <= kGroupTickets - 8) {      // (the last words serve other launches' tickets)
        g.slab = (float*)slab;
        g.tickets = tickets;
        return comic_gemm_group_launch(g, wg, st);
      }
      COMIC_REQUIRE(target > 1, "gemm_group: split-K scratch too small");
      target = target / 2;
    }
  }
};

int check_desc(const comic_decoder_desc* d) {
  COMIC_REQUIRE(d, "decoder: null descriptor");
  COMIC_REQUIRE(d->D > 0 && d->E > 0 && d->A > 0 && d->V > 1 && d->C > 0 && d->Cg > 0 && d->H > 0 && d->M > 0,
                "decoder: bad dimensions");
  const int cv = d->fm_projection == 0 ? d->C : d->D;
  COMIC_REQUIRE(d->Cv == cv, "decoder: Cv must be %d for fm_projection %d", cv, d->fm_projection);
  const int a = (d->fm_projection == 0 && !d->context_layer) ? d->C : d->D;
  COMIC_REQUIRE(d->A == a, "decoder: attention size A must be %d", a);
  COMIC_REQUIRE(d->cell >= COMIC_CELL_LSTM && d->cell <= COMIC_CELL_GRU, "decoder: unknown cell %d", d->cell);
  return 0;
}
int check_cell_params(const comic_decoder_desc* d, const comic_decoder_params* p) {
  COMIC_REQUIRE(p && p->K, "decoder: null cell kernel");
  if (d->cell == COMIC_CELL_LSTM) COMIC_REQUIRE(p->b, "decoder: LSTM needs its bias");
  if (d->cell == COMIC_CELL_LN_LSTM) COMIC_REQUIRE(p->cell_ln, "decoder: LN_LSTM needs cell_ln");
  if (d->cell == COMIC_CELL_GRU) COMIC_REQUIRE(p->b && p->K_c && p->b_c, "decoder: GRU needs b, K_c, b_c");
  return 0;
}

comic_attn_desc attn_desc(const comic_decoder_desc* d, int rows) {
  comic_attn_desc a;
  a.B = rows; a.M = d->M; a.D = d->D; a.H = d->H; a.Cv = d->Cv;
  a.method = d->method; a.prob = d->prob; a.tied = d->fm_projection == 2;
  return a;
}

// keys / values for `rows` feature maps (ops_rnn.py:440-477)
int memory_projections(const comic_decoder_desc* d, const comic_decoder_params* p, const float* fm, int rows,
                       float* keys, float* values_buf, const float** values, hipStream_t st) {
  RC(gemm_big(fm, p->W_m, keys, nullptr, rows * d->M, d->D, d->C, d->C, d->D, d->D, 0, 0, 0.f, st));
  if (d->fm_projection == 2) {
    *values = keys;
  } else if (d->fm_projection == 1) {
    RC(gemm_big(fm, p->W_v, values_buf, nullptr, rows * d->M, d->D, d->C, d->C, d->D, d->D, 0, 0, 0.f, st));
    *values = values_buf;
  } else {
    *values = fm;
  }
  return 0;
}

struct InitBufs {
  float *x, *xh, *g, *gates, *c_new;
  float *lnx = nullptr, *lnr = nullptr;      // LN_LSTM, training: normalised rows [rows][5D] and 1/std [rows][8] of the init step
};

// _get_rnn_init (model_base.py:651-689) -> c0,h0 [rows,D]
int rnn_init_fwd(const comic_decoder_desc* d, const comic_decoder_params* p, const float* im_embed, int rows,
                 const float* mask_init, InitBufs& ib, float* c0, float* h0, hipStream_t st) {
  const int D = d->D, EA = d->E + d->A;
  if (d->init_method == 1) {
    RC(gemm(im_embed, p->W_init, h0, nullptr, rows, D, d->Cg, d->Cg, D, D, 0, 0, 0.f, st));
    RC(fill(c0, 0.f, (long)rows * D, st));
    return 0;
  }
  RC(gemm(im_embed, p->W_init, ib.x, nullptr, rows, EA, d->Cg, d->Cg, EA, EA, 0, 0, 0.f, st));
  RC(comic_dropout_apply(ib.x, mask_init, d->keep_in, ib.xh, (int64_t)rows * EA, (void*)st));
  // zero initial state: only the first E+A rows of the cell's kernel(s) contribute
  if (d->cell == COMIC_CELL_LN_LSTM) {
    RC(gemm(ib.xh, p->K, ib.g, nullptr, rows, 4 * D, EA, EA, 4 * D, 4 * D, 0, 0, 0.f, st));
    return comic_ln_lstm_fwd(ib.g, 1, p->cell_ln, nullptr, nullptr, ib.gates, ib.lnx, ib.lnr, ib.c_new, nullptr, nullptr, 1.f,
                             nullptr, 0, c0, h0, rows, D, nullptr, 0, st);
  }
  if (d->cell == COMIC_CELL_GRU) {           // r*h = 0: the candidate sees [x ; 0]; gates / candidate kept in ib.gates
    float* g2 = ib.g + (size_t)rows * 2 * D;
    RC(gemm(ib.xh, p->K, ib.g, nullptr, rows, 2 * D, EA, EA, 2 * D, 2 * D, 0, 0, 0.f, st));
    RC(comic_gru_gates_fwd(ib.g, 1, p->b, nullptr, ib.xh, EA, ib.gates, 4 * D, nullptr, 0, rows, D, EA, st));
    RC(gemm(ib.xh, p->K_c, g2, nullptr, rows, D, EA, EA, D, D, 0, 0, 0.f, st));
    RC(comic_gru_out_fwd(g2, 1, p->b_c, ib.gates, 4 * D, nullptr, ib.gates + 2 * D, 4 * D, nullptr, nullptr, 1.f, nullptr, 0,
                         h0, nullptr, 0, rows, D, st));
    return fill(c0, 0.f, (long)rows * D, st);
  }
  RC(gemm(ib.xh, p->K, ib.g, p->b, rows, 4 * D, EA, EA, 4 * D, 4 * D, 0, 0, 0.f, st));
  RC(comic_lstm_gates_fwd(ib.g, nullptr, nullptr, ib.gates, ib.c_new, nullptr, nullptr, nullptr, 1.f, nullptr, 0, c0,
                          h0, rows, D, (void*)st));
  return 0;
}

// one wrapper step without dropout / imputing (inference)
struct StepBufs {
  float *xh, *g, *y, *q, *alpha, *ctx, *c2, *h2, *att2;
  float* xh2 = nullptr;                       // GRU: [x ; att ; r*h]
};
int infer_step(const comic_decoder_desc* d, const comic_decoder_params* p, const comic_attn_desc& ad,
               const float* keys, const float* values, const float* x, const float* c, const float* h,
               const float* att, StepBufs& sb, float* alpha_d_out, int rows, hipStream_t st) {
  const int D = d->D, E = d->E, A = d->A, Wd = E + A + D;
  hipLaunchKernelGGL(assemble_input_kernel, dim3(cdiv(rows * Wd, 256)), dim3(256), 0, st, x, att, h, nullptr, 1.f,
                     sb.xh, rows, E, A, D);
  COMIC_LAUNCH_CHECK("assemble_input");
  if (d->cell == COMIC_CELL_LN_LSTM) {
    RC(gemm(sb.xh, p->K, sb.g, nullptr, rows, 4 * D, Wd, Wd, 4 * D, 4 * D, 0, 0, 0.f, st));
    RC(comic_ln_lstm_fwd(sb.g, 1, p->cell_ln, c, h, nullptr, nullptr, nullptr, nullptr, sb.y, nullptr, 1.f, nullptr, 0, sb.c2,
                         sb.h2, rows, D, nullptr, 0, st));
  } else if (d->cell == COMIC_CELL_GRU) {
    float* ru = sb.g + (size_t)rows * 2 * D;             // sb.g: [rows][2D] product, then [rows][2D] r | u
    RC(gemm(sb.xh, p->K, sb.g, nullptr, rows, 2 * D, Wd, Wd, 2 * D, 2 * D, 0, 0, 0.f, st));
    RC(comic_gru_gates_fwd(sb.g, 1, p->b, h, sb.xh, Wd, ru, 2 * D, sb.xh2, Wd, rows, D, E + A, st));
    RC(gemm(sb.xh2, p->K_c, sb.q, nullptr, rows, D, Wd, Wd, D, D, 0, 0, 0.f, st));      // sb.q: free until the query product
    RC(comic_gru_out_fwd(sb.q, 1, p->b_c, ru, 2 * D, h, nullptr, 0, sb.y, nullptr, 1.f, nullptr, 0, sb.h2, nullptr, 0, rows, D,
                         st));
    RC(fill(sb.c2, 0.f, (long)rows * D, st));            // the state is h alone; c rides along as zeros
  } else {
    RC(gemm(sb.xh, p->K, sb.g, p->b, rows, 4 * D, Wd, Wd, 4 * D, 4 * D, 0, 0, 0.f, st));
    RC(comic_lstm_gates_fwd(sb.g, c, h, nullptr, nullptr, nullptr, sb.y, nullptr, 1.f, nullptr, 0, sb.c2, sb.h2, rows,
                            D, (void*)st));
  }
  RC(gemm(sb.y, p->W_q, sb.q, nullptr, rows, D, D, D, D, D, 0, 0, 0.f, st));
  RC(comic_attn_step_fwd(&ad, keys, values, sb.q, p->ln_g, p->ln_b, p->v, p->tau, nullptr, 1.f, sb.alpha,
                         alpha_d_out, sb.ctx, (void*)st));
  if (d->context_layer) {
    RC(gemm(sb.ctx, p->W_a, sb.att2, nullptr, rows, D, d->Cv, d->Cv, D, D, 0, 0, 0.f, st));
  }
  return 0;
}

// The same wrapper step on the fused kernels: operand prep (embedding + parent gather + concat),
// LSTM product + gates, query product left as split-K partials for the attention kernel.
// Reads the previous step's raw outputs (c_src, h_src, att_src) through `parent`.
// operands of the streaming step kernels (lstm_stream.hip): packed LSTM kernel, the step's operand rows and outputs as
// hi / lo fragments, packed W_q (null: exact split-K product)
struct StreamBufs {
  const void* kfrag;
  void* xfrag;
  void* yfrag;
  const void* wqfrag;
  int skip_prep = 0;       // the operand rows of this step were prepared by the previous step's beam merge
  // a second product over the same y, launched with the query projection (vocabulary projection at a small V):
  const void* wofrag = nullptr;   // packed W_o, or null
  int wo_N = 0;
  float* wo_part = nullptr;       // out: its K-slice partials (second half of the split-K scratch)
  int wo_S = 0;                   // out: their count
  int q_S = 0;                    // > 0: the query partials are already in the split-K scratch (they rode another launch)
};
// first half: operand prep + LSTM product + cell -> c2, h2, y (and y as fragments on the streaming path)
int infer_step_lstm(const comic_decoder_desc* d, const comic_decoder_params* p, const float* kpanel, const int32_t* ids,
                    const int32_t* parent, int W, const float* c_src, const float* h_src, const float* att_src,
                    StepBufs& sb, float* c_in, int rows, hipStream_t st, const StreamBufs* sm) {
  const int D = d->D, E = d->E, A = d->A, Wd = E + A + D;
  if (sm) {         // many rows: the kernel streamed once for all of them (lstm_stream.hip)
    RC(comic_lstm_stream_step(p->emb, ids, parent, W, att_src, h_src, c_src, sm->kfrag, p->b, sm->xfrag, c_in,
                              (float*)g_splitk_ws, kSplitKBytes, sb.c2, sb.h2, sb.y, sm->yfrag, rows, E, A, D, d->V, sm->skip_prep, st));
  } else {
    const long n = (long)rows * (Wd + D);
    hipLaunchKernelGGL(infer_prep_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, p->emb, ids, parent, W,
                       att_src, h_src, c_src, sb.xh, c_in, rows, E, A, D, d->V, g_comic_stop.p, g_comic_stop.t);
    COMIC_LAUNCH_CHECK("infer_prep");
    RC(comic_lstm_step_fused(sb.xh, Wd, kpanel, p->b, c_in, nullptr, nullptr, nullptr, sb.y, nullptr, 1.f, nullptr, 0,
                             sb.c2, sb.h2, nullptr, 0, rows, D, Wd, st));
  }
  return 0;
}
// second half: query projection (split-K partials in g_splitk_ws) + attention -> alpha, context (the next step's
// attention state); reads y, writes nothing the vocabulary projection of the step looks at
int infer_step_attend(const comic_decoder_desc* d, const comic_decoder_params* p, const comic_attn_desc& ad,
                      const float* keys, const float* values, StepBufs& sb, float* alpha_d_out, int rows, hipStream_t st,
                      StreamBufs* sm, int mem_div) {
  const int D = d->D;
  int S = 1;
  float* part = (float*)g_splitk_ws;
  if (sm && sm->q_S > 0) {
    S = sm->q_S;
  } else if (sm && sm->wqfrag && sm->wofrag) {
    sm->wo_part = (float*)((char*)g_splitk_ws + kSplitKBytes / 2);
    RC(comic_stream_gemm2(sm->yfrag, sm->wqfrag, part, D, &S, sm->wofrag, sm->wo_part, sm->wo_N, &sm->wo_S, kSplitKBytes / 2,
                          rows, D, st));
  } else if (sm && sm->wqfrag) RC(comic_stream_gemm(sm->yfrag, sm->wqfrag, part, kSplitKBytes, rows, D, D, &S, st));
  else RC(comic_gemm_f32_partial(sb.y, p->W_q, rows, D, D, D, D, 0, part, kSplitKBytes, &S, st));
  // large memories (Inception-V1 Mixed_4f: M = 196): the attention step in its split form; its [rows][H][M] scratch is the
  // pre-activation gate buffer, which the fused LSTM step never materialises
  float* attn_ws = ((long)d->H * d->M <= 4L * D) ? sb.g : nullptr;
  RC(comic_attn_fwd_ex(&ad, keys, values, part, p->ln_g, p->ln_b, p->v, p->tau, nullptr, 1.f, sb.alpha, alpha_d_out,
                       sb.ctx, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, 1.f, S, nullptr, attn_ws, st, mem_div));
  if (d->context_layer) {
    RC(gemm(sb.ctx, p->W_a, sb.att2, nullptr, rows, D, d->Cv, d->Cv, D, D, 0, 0, 0.f, st));
  }
  return 0;
}
int infer_step_fused(const comic_decoder_desc* d, const comic_decoder_params* p, const comic_attn_desc& ad,
                     const float* keys, const float* values, const float* kpanel, const int32_t* ids,
                     const int32_t* parent, int W, const float* c_src, const float* h_src, const float* att_src,
                     StepBufs& sb, float* c_in, float* alpha_d_out, int rows, hipStream_t st,
                     StreamBufs* sm = nullptr, int mem_div = 1) {
  RC(infer_step_lstm(d, p, kpanel, ids, parent, W, c_src, h_src, att_src, sb, c_in, rows, st, sm));
  return infer_step_attend(d, p, ad, keys, values, sb, alpha_d_out, rows, st, sm, mem_div);
}

}  // namespace

thread_local int g_train_path = 0;
extern "C" int comic_decoder_train_path(void) { return g_train_path; }
thread_local int g_greedy_path = 0;
extern "C" int comic_decoder_greedy_path(void) { return g_greedy_path; }
thread_local int g_beam_path = 0;
extern "C" int comic_decoder_beam_path(void) { return g_beam_path; }
thread_local int g_score_path = 0;
extern "C" int comic_decoder_score_path(void) { return g_score_path; }

namespace {

// ---- workspace of the teacher-forced step (training and scoring) ---------------------------------------------------------
// TrainLayout::carve is the ONE definition of the blocks, their order and their sizes: comic_decoder_train_workspace and
// comic_decoder_score_workspace run it over a null base, the step over the caller's buffer.  What a launch assumes about
// where blocks sit relative to each other is an accessor below: the step does no pointer arithmetic across blocks itself.
enum TfMode { TF_TRAIN, TF_SCORE };           // TF_SCORE: the backward-only blocks (x bw) are not taken (0 bytes)
struct TrainLayout {
  long B = 0, TB = 0, D = 0, A = 0, M = 0, H = 0, Wd = 0;
  size_t bytes = 0;           // what carve took; ok: it fitted the caller's buffer
  bool ok = false;
  InitBufs ib;
  int32_t* in_tb;
  float *keys, *values_buf;
  float *emb_all, *xh_all, *g_tmp, *gates_all, *cs, *hs, *cnew_all, *y_all, *q_all, *alpha_all, *ctx_all, *att_new, *att_all;
  float *dlogits, *wo_pad, *dy_all, *dq_all, *dg_all, *dxh, *dc, *dh, *datt, *datt_live, *dctx, *demb, *dkeys, *dvalues_buf;
  float *pgrad, *dmap, *dx_init, *kpanel_f, *kpanel_b, *wq_panel, *dq_part, *dg_blk, *dq_sum, *dstate, *pgrad4, *dotp, *statp;
  float *lnx_all = nullptr, *lnr_all = nullptr, *lnpg = nullptr, *cell_tmp = nullptr, *xh2_all = nullptr, *gru_dxh = nullptr;
  void *splitk_a, *splitk_b;                  // split-K partials of the main stream / of the second gradient lane
  unsigned* persist_sync;
  // scoring (latched flags: FlagScope): the alignment history when the caller takes none, and the projection's scratch (no
  // [T'][B][V] block on the streaming path: packed W_o and per-chunk partials)
  bool score_stream = false;
  float* attn_hist_own = nullptr;
  void* score_ws;
  int64_t score_ws_bytes = 0;

  void carve(const comic_decoder_desc* d, int B_, int T, TfMode mode, bool own_attn_hist, void* base, size_t cap) {
    Bump w(base, cap);
    B = B_; D = d->D; A = d->A; M = d->M; H = d->H; Wd = d->E + d->A + d->D; TB = (long)T * B;
    const long E = d->E, V = d->V, Cv = d->Cv, EA = E + A;
    const long bw = mode == TF_SCORE ? 0 : 1;
    keys = w.take<float>(B * M * D); values_buf = w.take<float>(B * M * D);
    ib.x = w.take<float>(B * EA); ib.xh = w.take<float>(B * EA);
    ib.g = w.take<float>(B * 4 * D); ib.gates = w.take<float>(B * 4 * D); ib.c_new = w.take<float>(B * D);
    emb_all = w.take<float>(bw * TB * E); in_tb = w.take<int32_t>(TB);
    xh_all = w.take<float>((TB + B) * Wd);                  // (+ the init step's operand rows: xh_init)
    g_tmp = w.take<float>(B * 4 * D); gates_all = w.take<float>(TB * 4 * D);
    cs = w.take<float>((TB + B) * D); hs = w.take<float>((TB + B) * D);
    cnew_all = w.take<float>(TB * D); y_all = w.take<float>(TB * D); q_all = w.take<float>(TB * D);
    alpha_all = w.take<float>(TB * H * M); ctx_all = w.take<float>(TB * Cv);
    att_new = w.take<float>(B * D); att_all = w.take<float>((TB + B) * A);
    const long Vp = (V + 3) / 4 * 4;                        // d logits / W_o rows padded to 16 bytes: every product loads them 16 bytes at a time
    dlogits = w.take<float>(bw * TB * Vp); wo_pad = w.take<float>(bw * D * Vp);
    dy_all = w.take<float>(bw * TB * D); dq_all = w.take<float>(bw * TB * D);
    dg_all = w.take<float>(bw * (TB + B) * 4 * D);          // (+ the init step's rows: dg_init)
    dxh = w.take<float>(bw * B * Wd);
    dc = w.take<float>(bw * B * D); dh = w.take<float>(bw * B * D); datt = w.take<float>(bw * B * A);   // consecutive: state_grads()
    datt_live = w.take<float>(bw * B * A); dctx = w.take<float>(bw * B * Cv); demb = w.take<float>(bw * TB * E);
    dkeys = w.take<float>(bw * B * M * D); dvalues_buf = w.take<float>(bw * B * M * Cv);
    pgrad = w.take<float>(bw * TB * (3 * D + 1));           // one attention-parameter gradient row per (step, batch row)
    dmap = w.take<float>(bw * TB * M); dx_init = w.take<float>(bw * B * EA);
    splitk_a = w.take<char>(kSplitKBytes); splitk_b = w.take<char>(kSplitKBytes);       // consecutive: gg_slab()
    kpanel_f = w.take<float>(comic_lstm_panel_floats((int)D, (int)Wd, 0));          // LSTM kernel panels (fused step)
    kpanel_b = w.take<float>(bw * comic_lstm_panel_floats((int)D, (int)Wd, 1)); wq_panel = w.take<float>(bw * D * D);
    persist_sync = w.take<unsigned>(kPersistSyncWords + kGroupTickets);     // persistent loops' sync words | gg_tickets()
    const long TB16 = (long)T * ((B + 15) / 16) * 16;
    dq_part = w.take<float>(TB * 4 * D);                    // persistent backward: d q partials; per-step kernels: attn_scratch()
    dg_blk = w.take<float>(bw * TB16 * 4 * D); dq_sum = w.take<float>(bw * TB16 * D);      // ... d gates, summed d q (blocked)
    dstate = w.take<float>(bw * TB * 2 * D);                // ... d att | d h
    pgrad4 = w.take<float>(bw * 4 * B * (3 * D + 1));       // ... its parameter-gradient rows
    dotp = w.take<float>(bw * TB * 64);                     // ... per-head dot products of the row quarters (M > 28)
    // forward loop, channel-quarter form: LayerNorm sums of the quarters
    statp = comic_persist_fwd_bigm((int)M, d->fm_projection == 2) ? w.take<float>(TB * 8 * M) : nullptr;
    if (d->cell == COMIC_CELL_LN_LSTM) {      // normalised rows, 1/std and LayerNorm gradient rows of every step + the init step
      lnx_all = w.take<float>((TB + B) * 5 * D); lnr_all = w.take<float>((TB + B) * 8);
      lnpg = w.take<float>(bw * (TB + B) * 10 * D); cell_tmp = w.take<float>(10 * D);
      ib.lnx = lnx_all + TB * 5 * D; ib.lnr = lnr_all + TB * 8;      // the init step's rows sit behind the time steps'
    } else if (d->cell == COMIC_CELL_GRU) {   // [x ; att ; r*h] of every step, the two d-operand products of a step, bias sums
      xh2_all = w.take<float>(TB * Wd); gru_dxh = w.take<float>(bw * 2 * B * Wd); cell_tmp = w.take<float>(4 * D);
    }
    score_stream = mode == TF_SCORE && beam_logits_enabled() && comic_score_stream_supported((int)D, (int)V);
    score_ws_bytes = mode == TF_SCORE ? comic_score_logits_ws_bytes((int)D, (int)V, TB, score_stream) : 0;
    if (mode == TF_SCORE && own_attn_hist) attn_hist_own = w.take<float>(TB * H * M);
    score_ws = w.take<char>((size_t)score_ws_bytes);
    bytes = w.off; ok = w.ok;
  }

  // row block Tp of xh_all / dg_all: the rnn init step's operand rows [drop(x_init) ; 0] and its d gates (grouped path)
  float* xh_init(int Tp) const { return xh_all + Tp * B * Wd; }
  float* dg_init(int Tp) const { return dg_all + Tp * B * 4 * D; }
  // dc | dh | datt are zeroed by ONE fill: consecutive blocks (the span includes their alignment padding)
  float* state_grads() const { return dc; }
  long state_grads_floats() const { return (long)((datt + B * A) - dc); }
  // scratch slab of the grouped launches: both lanes' split-K blocks, consecutive
  void* gg_slab() const { return splitk_a; }
  int64_t gg_slab_cap() const { return 2 * kSplitKBytes; }
  // tile tickets of the grouped launches: kGroupTickets words behind the persistent loops' sync words, zeroed with them by
  // comic_persist_prepare (sync_words() words) and left zero by every launch; the last one is the loss launch's
  int sync_words() const { return kPersistSyncWords + kGroupTickets; }
  unsigned* gg_tickets() const { return persist_sync + kPersistSyncWords; }
  unsigned* loss_ticket() const { return gg_tickets() + kGroupTickets - 1; }
  // scratch of the split attention kernels (large memories: comic_attn_splits workgroups per batch row; 2 x [B][H][M] +
  // comic_attn_bwd_scratch): the d q partials of the persistent backward loop, free whenever the per-step kernels run
  float* attn_scratch(bool persist_b) const {
    return (!persist_b && comic_attn_splits((int)B, (int)M) > 1 &&
            TB * 4 * D >= B * H * M + comic_attn_bwd_scratch((int)B, (int)H, (int)M, (int)D)) ? dq_part : nullptr;
  }
  float* attn_scratch_bwd(float* scratch) const { return scratch ? scratch + B * H * M : nullptr; }
  // partial sums of the map loss: dxh [B][Wd], free until the backward loop (the step checks that they fit)
  float* maploss_partials() const { return dxh; }
  long maploss_partials_cap() const { return B * Wd; }
  // column-summed [v | ln_g | ln_b | tau] row (lane form): g_tmp [B][4D], free after the loops, >= 3D + 1 floats at any B
  float* pgrad_sum() const { return g_tmp; }
};

// Caller's side of one teacher-forced call: what comic_decoder_train_step / comic_decoder_score were handed.  Scoring
// (score set): the forward with the masks absent, then the per-token log-likelihoods (score_logits.hip) in place of
// the logits product, the loss and the backward.
struct StepIO {
  const float *fm, *im_embed, *wmask_bt, *coef_bt, *mask_init_in, *mask_in, *mask_out, *mask_alpha;
  const int32_t *inputs_bt, *targets_bt, *lens;
  int B, T, Tp;
  float *logits_tb, *attn_hist, *loss_rows, *map_loss, *dfm, *dim_embed;
  int32_t* ids_tb;
  bool score;
  float *token_logp_tb, *caption_logp;        // [T][B], [B]: scoring
  void* workspace;
  int64_t workspace_bytes;
  const comic_soft_targets* soft;             // soft targets of the sequence loss, or null (comic_decoder_train_step_soft)
};

// The decisions of one call, taken once after validation
struct StepPlan {
  bool score, score_stream, use_map, drop_in;
  bool do_fwd, do_bwd;        // COMIC_DEC_PHASE_FWD / _BWD: the step in two calls over one workspace (to the logits | loss + backward)
  bool fused, fused_q;        // fused step kernels (decoder_fused.hip); ... of the backward's query half too
  bool persist, persist_b;    // the time loops as persistent launches (decoder_persist.hip, decoder_persist_bwd.hip)
  bool grp;                   // the products outside the time loops as grouped launches (gemm_group.hip)
  bool prologue_rides;        // the forward panel of the LSTM kernel and the padded W_o ride on comic_persist_prepare
  int attn_bwd_mode, Vp, ldl; // comic_attn_bwd_ex's pgrad_overwrite; padded vocabulary; row stride of d logits
  const float *wo_g, *values; // W_o with rows of ldl floats; the attention's values (keys when tied, fm without a projection)
  const float *m_init, *m_in, *m_out, *m_alpha;               // dropout masks: null when that dropout is off
  float *attn_hist, *attn_ws, *dvalues;
  comic_attn_desc ad;
  SideLane* lane;
};

// The pointers of time step t: the one place of the t * B * ... offsets, of "null when that dropout is off" and of "the next
// step's operand row, or null at the last step"
struct StepView {
  float *xh, *xh_next_att, *xh_next_h, *gates, *cnew, *y, *q, *alpha, *hist, *ctx, *c_next, *h_next, *att_next;
  const float *c_prev, *h_prev, *att_prev, *mask_in, *mask_att_next, *mask_out, *mask_alpha, *dmap;
  float *lnx, *lnr, *xh2, *lnpg;              // LN_LSTM / GRU rows (null for the other cells)
  float *dq, *dy, *dg, *demb, *pgrad;         // backward
};

struct TeacherForcedStep {
  const comic_decoder_desc* d;
  const comic_decoder_params *p, *gr;
  const StepIO& io;
  hipStream_t st;
  TrainLayout L{};
  StepPlan pl{};
  int B = 0, T = 0, Tp = 0, D = 0, E = 0, A = 0, V = 0, M = 0, H = 0, Cv = 0, EA = 0, Wd = 0, cell = 0;
  float* dx_im = nullptr;     // gradient w.r.t. (im_embed * W_init), n_init columns: set by the weight-gradient phase
  int n_init = 0;

  StepView view(int t) const {
    const size_t r = (size_t)t * B;             // first row of the step in the time-major blocks
    const bool last = t + 1 >= Tp;
    StepView v{};
    float* xh_n = last ? nullptr : L.xh_all + (r + B) * Wd;
    v.xh = L.xh_all + r * Wd; v.xh_next_att = xh_n ? xh_n + E : nullptr; v.xh_next_h = xh_n ? xh_n + EA : nullptr;
    v.gates = L.gates_all + r * 4 * D; v.cnew = L.cnew_all + r * D; v.y = L.y_all + r * D; v.q = L.q_all + r * D;
    v.alpha = L.alpha_all + r * H * M; v.hist = pl.attn_hist + r * H * M; v.ctx = L.ctx_all + r * Cv;
    v.c_prev = L.cs + r * D; v.h_prev = L.hs + r * D; v.att_prev = L.att_all + r * A;
    v.c_next = L.cs + (r + B) * D; v.h_next = L.hs + (r + B) * D; v.att_next = L.att_all + (r + B) * A;
    v.mask_in = pl.m_in ? pl.m_in + r * EA : nullptr; v.mask_att_next = (pl.m_in && !last) ? pl.m_in + (r + B) * EA + E : nullptr;
    v.mask_out = pl.m_out ? pl.m_out + r * D : nullptr; v.mask_alpha = pl.m_alpha ? pl.m_alpha + r * H * M : nullptr;
    v.lnx = L.lnx_all ? L.lnx_all + r * 5 * D : nullptr; v.lnr = L.lnr_all ? L.lnr_all + r * 8 : nullptr;
    v.xh2 = L.xh2_all ? L.xh2_all + r * Wd : nullptr;
    if (pl.score) return v;
    v.lnpg = L.lnpg ? L.lnpg + r * 10 * D : nullptr; v.dmap = pl.use_map ? L.dmap + r * M : nullptr;
    v.dq = L.dq_all + r * D; v.dy = L.dy_all + r * D; v.dg = L.dg_all + r * 4 * D; v.demb = L.demb + r * E;
    v.pgrad = L.pgrad + r * (3 * D + 1);
    return v;
  }

  // ---- validation, workspace, plan ---------------------------------------------------------------------------------------
  int validate_and_plan() {
    const bool sc = io.score;
    if (!sc) {
      COMIC_REQUIRE(p && gr && io.fm && io.im_embed && io.inputs_bt && io.targets_bt && io.wmask_bt && io.coef_bt && io.lens,
                    "train_step: null input");
      COMIC_REQUIRE(io.logits_tb && io.ids_tb && io.attn_hist && io.loss_rows && io.map_loss && io.workspace,
                    "train_step: null output");
    } else {
      COMIC_REQUIRE(p && io.fm && io.im_embed && io.inputs_bt && io.targets_bt && io.wmask_bt && io.lens, "score: null input");
      COMIC_REQUIRE(io.token_logp_tb && io.caption_logp && io.workspace, "score: null output");
    }
    B = io.B; T = io.T; Tp = io.Tp;
    COMIC_REQUIRE(B > 0 && T > 0 && Tp > 0 && Tp <= T, "train_step: bad B/T/Tp (%d %d %d)", B, T, Tp);
    if (!sc) COMIC_REQUIRE(io.workspace_bytes >= comic_decoder_train_workspace(d, B, T), "train_step: workspace too small");
    COMIC_REQUIRE(d->keep_in >= 1.f || (io.mask_in && (d->init_method == 1 || io.mask_init_in)),
                  "train_step: input dropout enabled but no mask given");
    COMIC_REQUIRE(d->keep_out >= 1.f || io.mask_out, "train_step: output dropout enabled but no mask given");
    COMIC_REQUIRE(d->keep_alpha >= 1.f || io.mask_alpha, "train_step: attention dropout enabled but no mask given");
    D = d->D; E = d->E; A = d->A; V = d->V; M = d->M; H = d->H; Cv = d->Cv; EA = E + A; Wd = E + A + D; cell = d->cell;
    L.carve(d, B, T, sc ? TF_SCORE : TF_TRAIN, !io.attn_hist, io.workspace, (size_t)io.workspace_bytes);
    g_splitk_ws = L.splitk_a;
    COMIC_REQUIRE(L.ok, sc ? "score: workspace too small" : "train_step: workspace overflow");
    RC(check_cell_params(d, p));
    pl.score = sc;
    pl.do_fwd = !(d->flags & COMIC_DEC_PHASE_BWD); pl.do_bwd = !(d->flags & COMIC_DEC_PHASE_FWD);
    COMIC_REQUIRE(pl.do_fwd || pl.do_bwd, "train_step: both phase flags set");
    pl.ad = attn_desc(d, B);
    pl.values = d->fm_projection == 2 ? L.keys : d->fm_projection == 1 ? L.values_buf : io.fm;   // (= what memory_projections reports)
    pl.drop_in = d->keep_in < 1.f;
    pl.m_init = pl.drop_in ? io.mask_init_in : nullptr; pl.m_in = pl.drop_in ? io.mask_in : nullptr;
    pl.m_out = d->keep_out < 1.f ? io.mask_out : nullptr; pl.m_alpha = d->keep_alpha < 1.f ? io.mask_alpha : nullptr;
    pl.attn_hist = io.attn_hist ? io.attn_hist : L.attn_hist_own;
    pl.score_stream = L.score_stream;
    pl.fused = fused_step_enabled() && comic_fused_step_supported(D, Wd);
    pl.fused_q = pl.fused && D % 16 == 0;
    pl.persist = pl.fused && persist_enabled() &&
                 comic_persist_fwd_supported(B, D, E, A, M, H, Cv, d->method, d->context_layer, pl.ad.tied) &&
                 comic_persist_fits_device(B);
    pl.persist_b = !sc && pl.persist && persist_bwd_enabled() &&
                   comic_persist_bwd_supported(B, D, E, A, M, H, Cv, d->method, d->prob, d->context_layer, pl.ad.tied);
    if (sc) g_score_path = (pl.persist ? 1 : 0) | (pl.score_stream ? 2 : 0);
    else g_train_path = (pl.persist ? 1 : 0) | (pl.persist_b ? 2 : 0);
    pl.attn_ws = L.attn_scratch(pl.persist_b);
    pl.prologue_rides = pl.persist && pl.do_fwd && group_gemm_enabled() && cell == COMIC_CELL_LSTM && pl.fused;
    // grp: the rnn init step then keeps its operand rows and its d gates in row block Tp of xh_all / dg_all, so that d K and
    // d b are ONE product over (Tp + 1) * B rows.  (Products with a short reduction -- a handful of rows in all -- keep the
    // separate launches, whose small shapes run the exact-fp32 kernels: gemm_big's rule)
    pl.grp = group_gemm_enabled() && cell == COMIC_CELL_LSTM && (long)Tp * B >= 64 && (long)B * M >= 64 && B >= 16;
    pl.Vp = (V + 3) / 4 * 4;
    pl.ldl = pl.grp ? pl.Vp : V;
    pl.wo_g = (pl.grp && pl.Vp != V) ? L.wo_pad : p->W_o;
    pl.lane = pl.grp ? nullptr : side_lane();
    pl.use_map = d->map_loss_scale > 0.f;
    pl.dvalues = d->fm_projection != 2 ? L.dvalues_buf : L.dkeys;
    // softmax attention: the backward kernel runs as two workgroups per batch row (half of the memory rows each), whose
    // d q / parameter-gradient contributions are added into zero-filled rows (comic_attn_bwd_ex, pgrad_overwrite 2)
    pl.attn_bwd_mode = (d->prob == 0 && split_attn_bwd_enabled()) ? 2 : 1;
    return 0;
  }

  // ---- persistent loops: every hand-off buffer of the step starts as "not written yet", the sync words and tickets as zero
  int prologue() {
    ComicPersistRanges pr{};
    const long n16 = (long)Tp * ((B + 15) / 16) * 16 * D;
    pr.p[0] = L.xh_all; pr.n[0] = (long)Tp * B * Wd;
    pr.p[1] = L.y_all; pr.n[1] = (long)Tp * B * D;
    pr.p[2] = L.q_all; pr.n[2] = (long)Tp * B * D;
    if (L.statp) {                     // the quarters' partial LayerNorm sums (decoder_persist.hip, BIGM): [Tp][B][4][M/2][4]
      pr.p[8] = L.statp; pr.n[8] = (long)Tp * B * 8 * M;
    }
    if (pl.persist_b) {
      pr.p[3] = L.dq_part; pr.n[3] = (long)Tp * B * 4 * D;
      pr.p[4] = L.dg_blk; pr.n[4] = 4 * n16;
      pr.p[5] = L.dstate; pr.n[5] = (long)Tp * B * 2 * D;
      pr.p[6] = L.dq_sum; pr.n[6] = n16;
      pr.p[7] = L.dotp; pr.n[7] = (long)Tp * B * 64;
    }
    ComicPrologueExtra px{};
    if (pl.prologue_rides) {
      px.K = p->K; px.panel = L.kpanel_f; px.D = D; px.Wd = Wd; px.n_pack = comic_lstm_panel_floats(D, Wd, 0);
      if (pl.Vp != V && !pl.score) { px.W_o = p->W_o; px.wo_pad = L.wo_pad; px.V = V; px.Vp = pl.Vp; px.n_pad = (long)D * pl.Vp; }
    }
    return comic_persist_prepare(pr, L.persist_sync, L.sync_words(), st, pl.prologue_rides ? &px : nullptr);
  }

  // ---- forward set-up: weight panels, memory projections, rnn init -- as grouped launches ...
  int forward_setup_grouped() {
    const bool no_bwd_panels = pl.persist_b || pl.score;    // the persistent backward reads K and W_q in place
    if (!pl.persist)
      COMIC_REQUIRE(hipMemsetAsync(L.gg_tickets(), 0, sizeof(unsigned) * kGroupTickets, st) == hipSuccess, "train_step: memset");
    if (pl.fused && !(pl.prologue_rides && no_bwd_panels))
      RC(comic_pack_lstm_panels(p->K, pl.prologue_rides ? nullptr : L.kpanel_f, no_bwd_panels ? nullptr : L.kpanel_b, D, Wd, st));
    if (pl.fused_q && !no_bwd_panels) RC(comic_pack_wq_panel(p->W_q, L.wq_panel, D, st));
    if (pl.Vp != V && !pl.prologue_rides && !pl.score) {
      const long n = (long)D * pl.Vp;
      hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, p->W_o, L.wo_pad, V, pl.Vp, n);
      COMIC_LAUNCH_CHECK("pad W_o");
    }
    GemmGroupRun g1;
    g1.add(COMIC_GG_NN, io.fm, p->W_m, L.keys, B * M, D, d->C, d->C, D, D);
    if (d->fm_projection == 1) g1.add(COMIC_GG_NN, io.fm, p->W_v, L.values_buf, B * M, D, d->C, d->C, D, D);
    if (d->init_method == 1) {
      g1.add(COMIC_GG_NN, io.im_embed, p->W_init, L.hs, B, D, d->Cg, d->Cg, D, D);
    } else {
      ComicGemmProb* q = g1.add(COMIC_GG_NN, io.im_embed, p->W_init, L.xh_init(Tp), B, EA, d->Cg, d->Cg, EA, Wd);
      if (pl.drop_in) { q->mask = io.mask_init_in; q->ld_mask = EA; q->keep = d->keep_in; }
    }
    RC(g1.run(L.gg_slab(), L.gg_slab_cap(), L.gg_tickets(), st));
    if (d->init_method == 1) return fill(L.cs, 0.f, (long)B * D, st);
    // zero initial state: only the first E+A rows of the cell's kernel contribute
    GemmGroupRun g2;
    g2.add(COMIC_GG_NN, L.xh_init(Tp), p->K, L.ib.g, B, 4 * D, EA, Wd, 4 * D, 4 * D)->bias = p->b;
    return g2.run(L.gg_slab(), L.gg_slab_cap(), L.gg_tickets(), st);      // (the cell itself: inside the operand-row launch)
  }
  // ... or on two lanes: the panels (needed by the time loop only) and the rnn init on the side lane
  int forward_setup_lanes() {
    const bool no_bwd_panels = pl.persist_b || pl.score;
    LaneScope lane(pl.lane, st, L.splitk_b);
    RC(lane.rc);
    hipStream_t sl = lane.lane();
    if (pl.fused) RC(comic_pack_lstm_panels(p->K, L.kpanel_f, no_bwd_panels ? nullptr : L.kpanel_b, D, Wd, sl));
    if (pl.fused_q && !no_bwd_panels) RC(comic_pack_wq_panel(p->W_q, L.wq_panel, D, sl));
    RC(rnn_init_fwd(d, p, io.im_embed, B, pl.m_init, L.ib, L.cs, L.hs, sl));
    lane.main_ws();
    const float* values = nullptr;
    RC(memory_projections(d, p, io.fm, B, L.keys, L.values_buf, &values, st));
    return lane.join();
  }

  // operand rows before the loop: the x part of every step (embedding lookup + input dropout, hoisted) and step 0's att part
  // (zero: dropout of 0 is 0) and h part (h0); grouped path: the init step's cell from its zero state too
  int operand_rows() {
    const bool zi = pl.grp && d->init_method != 1;
    const long n = (long)Tp * B * E + (long)B * A + (long)B * D * (zi ? 2 : 1);
    hipLaunchKernelGGL(embed_step0_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, p->emb, io.inputs_bt, L.in_tb,
                       pl.m_in, d->keep_in, L.xh_all, L.att_all, L.hs, Tp, B, T, E, A, D, V,
                       zi ? L.xh_init(Tp) : (float*)nullptr, zi ? L.ib.g : (const float*)nullptr, L.ib.gates, L.ib.c_new, L.cs,
                       L.hs);
    COMIC_LAUNCH_CHECK("embed_step0");
    return 0;
  }

  // a persistent launch serves up to four 16-row groups of the batch (256 CUs)
  template <typename Args>
  int launch_groups(Args& a, int (*launch)(const Args&, hipStream_t)) {
    const int n_grp = (B + 15) / 16;
    for (a.grp0 = 0; a.grp0 < n_grp; a.grp0 += 4) {
      a.n_groups = std::min(4, n_grp - a.grp0);
      RC(launch(a, st));
    }
    return 0;
  }

  // ---- forward time loop, as persistent launches ...
  int forward_persistent() {
    ComicPersistFwdArgs pa{};
    pa.K_panel = L.kpanel_f; pa.bias = p->b; pa.W_q = p->W_q; pa.keys = L.keys; pa.values = pl.values;
    pa.ln_g = p->ln_g; pa.ln_b = p->ln_b; pa.v = p->v; pa.tau = p->tau; pa.lens = io.lens;
    pa.mask_in = pl.m_in; pa.mask_out = pl.m_out; pa.mask_alpha = pl.m_alpha;
    pa.keep_in = d->keep_in; pa.keep_out = d->keep_out; pa.keep_alpha = d->keep_alpha;
    pa.xh_all = L.xh_all; pa.gates_all = L.gates_all; pa.cnew_all = L.cnew_all; pa.y_all = L.y_all; pa.q_all = L.q_all;
    pa.cs = L.cs; pa.hs = L.hs; pa.att_all = L.att_all; pa.alpha_all = L.alpha_all; pa.attn_hist = pl.attn_hist;
    pa.ctx_all = L.ctx_all; pa.sync = L.persist_sync;
    pa.statp = L.statp;
    pa.B = B; pa.D = D; pa.E = E; pa.Wd = Wd; pa.M = M; pa.H = H; pa.Tp = Tp;
    pa.method = d->method; pa.prob = d->prob; pa.tied = pl.ad.tied;
    return launch_groups(pa, comic_persist_fwd_launch);
  }

  // the recurrent cell of step t in its per-step forms: the fused LSTM step, or a split-K product + the cell's kernel(s)
  int cell_fwd(const StepView& v, int t) {
    float* part = (float*)g_splitk_ws;
    int S = 1;
    if (pl.fused)
      return comic_lstm_step_fused(v.xh, Wd, L.kpanel_f, p->b, v.c_prev, v.h_prev, v.gates, v.cnew, v.y, v.mask_out, d->keep_out,
                                   io.lens, t, v.c_next, v.h_next, v.xh_next_h, Wd, B, D, Wd, st);
    if (cell == COMIC_CELL_GRU) {                // gates_all[t]: r | u | candidate | -
      RC(comic_gemm_f32_partial(v.xh, p->K, B, 2 * D, Wd, Wd, 2 * D, 0, part, kSplitKBytes, &S, st));
      RC(comic_gru_gates_fwd(part, S, p->b, v.h_prev, v.xh, Wd, v.gates, 4 * D, v.xh2, Wd, B, D, EA, st));
      RC(comic_gemm_f32_partial(v.xh2, p->K_c, B, D, Wd, Wd, D, 0, part, kSplitKBytes, &S, st));
      return comic_gru_out_fwd(part, S, p->b_c, v.gates, 4 * D, v.h_prev, v.gates + 2 * D, 4 * D, v.y, v.mask_out, d->keep_out,
                               io.lens, t, v.h_next, v.xh_next_h, Wd, B, D, st);
    }
    RC(comic_gemm_f32_partial(v.xh, p->K, B, 4 * D, Wd, Wd, 4 * D, 0, part, kSplitKBytes, &S, st));
    if (cell == COMIC_CELL_LN_LSTM)
      return comic_ln_lstm_fwd(part, S, p->cell_ln, v.c_prev, v.h_prev, v.gates, v.lnx, v.lnr, v.cnew, v.y, v.mask_out,
                               d->keep_out, io.lens, t, v.c_next, v.h_next, B, D, v.xh_next_h, Wd, st);
    return comic_lstm_gates_fwd_ex(part, v.c_prev, v.h_prev, v.gates, v.cnew, v.y, v.mask_out, d->keep_out, io.lens, t, v.c_next,
                                   v.h_next, B, D, v.xh_next_h, Wd, S, p->b, st);
  }
  // ... or per step: cell, query product (split-K partials), attention (+ the context layer)
  int forward_steps() {
    float* part = (float*)g_splitk_ws;
    for (int t = 0; t < Tp; ++t) {
      const StepView v = view(t);
      int S2 = 1;
      RC(cell_fwd(v, t));
      RC(comic_gemm_f32_partial(v.y, p->W_q, B, D, D, D, D, 0, part, kSplitKBytes, &S2, st));
      if (!d->context_layer) {
        RC(comic_attn_fwd_ex(&pl.ad, L.keys, pl.values, part, p->ln_g, p->ln_b, p->v, p->tau, v.mask_alpha, d->keep_alpha, v.alpha,
                             v.hist, v.ctx, io.lens, t, v.att_prev, v.att_next, v.xh_next_att, Wd, v.mask_att_next, EA,
                             d->keep_in, S2, v.q, pl.attn_ws, st));
      } else {
        RC(comic_attn_fwd_ex(&pl.ad, L.keys, pl.values, part, p->ln_g, p->ln_b, p->v, p->tau, v.mask_alpha, d->keep_alpha, v.alpha,
                             v.hist, v.ctx, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, 1.f, S2, v.q, pl.attn_ws, st));
        RC(gemm(v.ctx, p->W_a, L.att_new, nullptr, B, D, Cv, Cv, D, D, 0, 0, 0.f, st));
        hipLaunchKernelGGL(select_att_kernel, dim3(cdiv(B * A, 256)), dim3(256), 0, st, v.att_prev, (const float*)L.att_new,
                           io.lens, t, v.att_next, v.xh_next_att, Wd, v.mask_att_next, EA, d->keep_in, B, A);
        COMIC_LAUNCH_CHECK("select_att");
      }
    }
    return 0;
  }

  // ---- scoring tail: per-token log-likelihoods instead of logits / loss / backward; a timed-out loop turns them into NaN
  int score_tail() {
    if (!pl.score_stream)
      RC(gemm_big(L.y_all, p->W_o, comic_score_logits_buffer(L.score_ws), p->b_o, Tp * B, V, D, D, V, V, 0, 0, 0.f, st));
    RC(comic_score_logits(L.y_all, p->W_o, p->b_o, io.targets_bt, io.wmask_bt, io.lens, pl.persist ? L.persist_sync : nullptr, B,
                          T, Tp, D, V, pl.score_stream ? 1 : 0, io.token_logp_tb, io.caption_logp, L.score_ws, L.score_ws_bytes,
                          st));
    COMIC_LAUNCH_CHECK("score");
    return 0;
  }

  // ---- output projection for all executed steps
  int logits() {
    if (!pl.grp) return gemm_big(L.y_all, p->W_o, io.logits_tb, p->b_o, Tp * B, V, D, D, V, V, 0, 0, 0.f, st);
    GemmGroupRun go;
    go.add(COMIC_GG_NN, L.y_all, pl.wo_g, io.logits_tb, Tp * B, V, D, D, pl.ldl, V)->bias = p->b_o;
    return go.run(L.gg_slab(), L.gg_slab_cap(), L.gg_tickets(), st);
  }

  // ---- sequence loss + d logits, attention-map loss, padding of the steps past Tp
  int loss_and_padding() {
    const long n = (long)Tp * B * M;
    const int nparts = (int)cdiv64(n, 256);               // partial sums of the map loss
    const comic_soft_targets* soft = io.soft;
    if (soft) {         // soft targets: their own launch on either layout of d logits; the map loss as its two launches below
      RC(comic_xent_soft_ex(io.logits_tb, io.targets_bt, io.coef_bt, io.wmask_bt, io.lens, io.loss_rows, soft->nll_rows, L.dlogits,
                            pl.ldl, io.ids_tb, Tp, T, B, V, soft->smoothing, soft->teacher_weight, soft->K, soft->ids_tbk,
                            soft->probs_tbk, st));
    } else if (pl.grp) {       // both losses in one launch (d logits rows are ldl floats apart)
      COMIC_REQUIRE(nparts <= L.maploss_partials_cap(), "train_step: map-loss scratch too small");
      RC(comic_xent_maploss(io.logits_tb, io.targets_bt, io.coef_bt, io.wmask_bt, io.lens, io.loss_rows, L.dlogits, pl.ldl,
                            io.ids_tb, Tp, T, B, V, pl.attn_hist, L.dmap, L.maploss_partials(), io.map_loss, L.loss_ticket(), H, M,
                            d->map_loss_scale, st));
    } else {
      RC(comic_xent_ex(io.logits_tb, io.targets_bt, io.coef_bt, io.wmask_bt, io.lens, io.loss_rows, L.dlogits, io.ids_tb, Tp, T, B,
                       V, st));
    }
    for (int t = Tp; t < T; ++t) {  // ops_rnn.py:235-241: pad by copying the last executed step
      (void)hipMemcpyAsync(io.logits_tb + (size_t)t * B * V, io.logits_tb + (size_t)(Tp - 1) * B * V, sizeof(float) * B * V,
                           hipMemcpyDeviceToDevice, st);
      (void)hipMemcpyAsync(io.ids_tb + (size_t)t * B, io.ids_tb + (size_t)(Tp - 1) * B, sizeof(int32_t) * B,
                           hipMemcpyDeviceToDevice, st);
      RC(fill(io.loss_rows + (size_t)t * B, 0.f, B, st));
      if (soft && soft->nll_rows) RC(fill(soft->nll_rows + (size_t)t * B, 0.f, B, st));
    }
    if (!pl.grp || soft) {
      float* partial = L.maploss_partials();
      COMIC_REQUIRE(nparts <= L.maploss_partials_cap(), "train_step: map-loss scratch too small");
      hipLaunchKernelGGL(maploss_part_kernel, dim3(nparts), dim3(256), 0, st, (const float*)pl.attn_hist, L.dmap, partial, Tp, B,
                         H, M, d->map_loss_scale);
      hipLaunchKernelGGL(maploss_final_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, nparts, n, d->map_loss_scale,
                         io.map_loss);
      COMIC_LAUNCH_CHECK("maploss");
    }
    return 0;
  }

  // ---- backward: zero-fills of the per-step form, dy_all = dlogits * W_o^T (d W_o, d b_o: with the weight gradients)
  int backward_prepare() {
    if (!pl.persist_b) {
      RC(fill(L.dkeys, 0.f, (long)B * M * D, st));
      if (d->fm_projection != 2) RC(fill(L.dvalues_buf, 0.f, (long)B * M * Cv, st));
      RC(fill(L.state_grads(), 0.f, L.state_grads_floats(), st));
    }
    if (pl.grp) {
      GemmGroupRun gy;
      gy.add(COMIC_GG_NT, L.dlogits, pl.wo_g, L.dy_all, Tp * B, D, pl.ldl, pl.ldl, pl.ldl, D);     // (K = padded columns: zeros on both sides)
      RC(gy.run(L.gg_slab(), L.gg_slab_cap(), L.gg_tickets(), st));
    } else {
      RC(gemm_big(L.dlogits, p->W_o, L.dy_all, nullptr, Tp * B, D, V, V, V, D, 0, 1, 0.f, st));
    }
    if (d->context_layer) RC(fill(gr->W_a, 0.f, (long)Cv * D, st));
    return 0;
  }

  // ---- backward time loop, as persistent launches ...
  int backward_persistent() {
    // M > 64: the loop ADDS its rows' d keys into memory step by step (one writer per address, in step order)
    const bool own_rows = (d->flags & COMIC_DEC_BWD_OWN_ROWS) != 0;
    if (M > 64 || own_rows) RC(fill(L.dkeys, 0.f, (long)B * M * D, st));
    ComicPersistBwdArgs pb{};
    pb.own_rows = own_rows ? 1 : 0;
    pb.K = p->K; pb.W_q = p->W_q; pb.keys = L.keys;
    pb.ln_g = p->ln_g; pb.ln_b = p->ln_b; pb.v = p->v; pb.tau = p->tau; pb.lens = io.lens;
    pb.mask_in = pl.m_in; pb.mask_out = pl.m_out; pb.mask_alpha = pl.m_alpha;
    pb.keep_in = d->keep_in; pb.keep_out = d->keep_out; pb.keep_alpha = d->keep_alpha;
    pb.q_all = L.q_all; pb.alpha_all = L.alpha_all; pb.gates_all = L.gates_all; pb.cs = L.cs; pb.cnew_all = L.cnew_all;
    pb.dy_all = L.dy_all; pb.dmap = pl.use_map ? L.dmap : nullptr;
    pb.dq_part = L.dq_part; pb.dq_sum = L.dq_sum; pb.dg_blk = L.dg_blk; pb.dg_all = L.dg_all; pb.dstate = L.dstate;
    pb.dotp = L.dotp;
    pb.dq_all = L.dq_all; pb.dc = L.dc; pb.dh = L.dh; pb.dkeys = L.dkeys; pb.pgrad = L.pgrad4; pb.sync = L.persist_sync;
    pb.B = B; pb.E = E; pb.M = M; pb.H = H; pb.Tp = Tp; pb.method = d->method;
    return launch_groups(pb, comic_persist_bwd_launch);
  }

  // d (attention state after step t) -> d q, d keys / values, parameter-gradient row; `carry` for the operand backward
  int attention_bwd(const StepView& v, int t, int* carry) {
    const bool cl = d->context_layer;
    *carry = cl ? 0 : 1;
    if (cl) {                   // the live rows' d(att state) through the context layer -> d ctx
      hipLaunchKernelGGL(split_live_kernel, dim3(cdiv(B * A, 256)), dim3(256), 0, st, L.datt, L.datt_live, io.lens, t, B, A);
      COMIC_LAUNCH_CHECK("split_live");
      RC(gemm(v.ctx, L.datt_live, gr->W_a, nullptr, Cv, D, B, Cv, D, D, 1, 0, 1.f, st));
      RC(gemm(L.datt_live, p->W_a, L.dctx, nullptr, B, Cv, D, D, D, Cv, 0, 1, 0.f, st));
    }                           // else: attn_bwd masks d(att state) by "live" itself; input_bwd keeps the finished rows' share
    return comic_attn_bwd_ex(&pl.ad, L.keys, pl.values, v.q, p->ln_g, p->ln_b, p->v, p->tau, v.alpha, v.mask_alpha, d->keep_alpha,
                             cl ? L.dctx : L.datt, v.dmap, v.dq, L.dkeys, pl.dvalues, v.pgrad, cl ? nullptr : io.lens, cl ? 0 : t, st,
                             pl.attn_bwd_mode, pl.attn_ws, L.attn_scratch_bwd(pl.attn_ws));
  }
  // ... or per step: attention backward, the cell's gates, d operand row -> d emb, d att, d h
  int backward_steps() {
    if (pl.attn_bwd_mode == 2) {
      RC(fill(L.dq_all, 0.f, (long)Tp * B * D, st));
      RC(fill(L.pgrad, 0.f, (long)Tp * B * (3 * D + 1), st));
    }
    float* part = (float*)g_splitk_ws;
    for (int t = Tp - 1; t >= 0; --t) {
      const StepView v = view(t);
      int carry, S3 = 1, S4 = 1;
      const float* dxh_t = part;                 // d operand row(s) of the step: S4 slices
      RC(attention_bwd(v, t, &carry));
      if (pl.fused_q) {
        RC(comic_lstm_grad_fused(v.dq, L.wq_panel, v.gates, v.c_prev, v.cnew, v.dy, v.mask_out, d->keep_out, io.lens, t, L.dc,
                                 L.dh, v.dg, B, D, st));
      } else {
        RC(comic_gemm_f32_partial(v.dq, p->W_q, B, D, D, D, D, 1, part, kSplitKBytes, &S3, st));
        if (cell == COMIC_CELL_LN_LSTM) {
          RC(comic_ln_lstm_bwd(v.gates, v.lnx, v.lnr, p->cell_ln, v.c_prev, v.cnew, v.dy, part, S3, v.mask_out, d->keep_out,
                               io.lens, t, L.dc, L.dh, v.dg, v.lnpg, B, D, st));
        } else if (cell == COMIC_CELL_GRU) {       // dg_t: d r_pre | d u_pre | d candidate_pre | -
          float* slice1 = L.gru_dxh + (size_t)B * Wd;
          RC(comic_gru_bwd1(v.dy, part, S3, v.mask_out, d->keep_out, io.lens, t, L.dh, v.gates, 4 * D, v.gates + 2 * D, 4 * D,
                            v.h_prev, v.dg, 4 * D, B, D, st));
          RC(gemm(v.dg + 2 * D, p->K_c, slice1, nullptr, B, Wd, D, 4 * D, D, Wd, 0, 1, 0.f, st));
          RC(comic_gru_bwd2(slice1, Wd, v.gates, 4 * D, v.h_prev, v.dg, 4 * D, B, D, EA, st));
          RC(gemm(v.dg, p->K, L.gru_dxh, nullptr, B, Wd, 2 * D, 4 * D, 2 * D, Wd, 0, 1, 0.f, st));
          dxh_t = L.gru_dxh;                       // the two products are the two "split-K" slices input_bwd adds
          S4 = 2;
        } else {
          RC(comic_lstm_gates_bwd_ex(v.gates, v.c_prev, v.cnew, v.dy, part, S3, v.mask_out, d->keep_out, io.lens, t, L.dc, L.dh,
                                     v.dg, B, D, st));
        }
      }
      if (pl.fused) {
        RC(comic_input_grad_fused(v.dg, L.kpanel_b, v.mask_in, d->keep_in, v.demb, L.datt, L.dh, io.lens, t, carry, B, E, A, D, st));
        continue;
      }
      if (cell != COMIC_CELL_GRU) RC(comic_gemm_f32_partial(v.dg, p->K, B, Wd, 4 * D, 4 * D, 4 * D, 1, part, kSplitKBytes, &S4, st));
      hipLaunchKernelGGL(input_bwd_kernel, dim3(cdiv(B * Wd, 256)), dim3(256), 0, st, dxh_t, v.mask_in, d->keep_in, v.demb, L.datt,
                         L.dh, io.lens, t, carry, B, E, A, D, S4);
      COMIC_LAUNCH_CHECK("input_bwd");
    }
    return 0;
  }

  // ---- gradients that do not feed the recurrence, as ONE grouped launch: every weight gradient, the bias sums, the embedding
  // third of d gates * K^T, d x_init (and a second launch for what depends on d x_init / accumulates into dfm)
  int weight_grads_grouped() {
    const bool init_step = d->init_method != 1;
    const int rows_k = (Tp + (init_step ? 1 : 0)) * B;            // rows of the LSTM operand / d gates matrices
    float* dg_init = L.dg_init(Tp);
    if (init_step)                                               // d gates of the init step -> row block Tp of dg_all
      RC(comic_lstm_gates_bwd(L.ib.gates, nullptr, L.ib.c_new, nullptr, nullptr, 1.f, nullptr, 0, L.dc, L.dh, dg_init, B, D, (void*)st));
    GemmGroupRun g1, g2;
    g1.add(COMIC_GG_TN, L.xh_all, L.dg_all, gr->K, Wd, 4 * D, rows_k, Wd, 4 * D, 4 * D);
    g1.add(COMIC_GG_TN, io.fm, L.dkeys, gr->W_m, d->C, D, B * M, d->C, D, D);
    if (d->fm_projection == 1) g1.add(COMIC_GG_TN, io.fm, L.dvalues_buf, gr->W_v, d->C, D, B * M, d->C, D, D);
    if (pl.persist_b) {   // the embedding third of d gates * K^T, all steps at once, and its input dropout
      ComicGemmProb* q = g1.add(COMIC_GG_NT, L.dg_all, p->K, L.demb, Tp * B, E, 4 * D, 4 * D, 4 * D, E);
      if (pl.drop_in) { q->mask = io.mask_in; q->ld_mask = EA; q->keep = d->keep_in; }
    }
    g1.add(COMIC_GG_TN, L.y_all, L.dq_all, gr->W_q, D, D, Tp * B, D, D, D);
    g1.add(COMIC_GG_TN, L.y_all, L.dlogits, gr->W_o, D, V, Tp * B, D, pl.ldl, V);
    if (io.dfm) g1.add(COMIC_GG_NT, L.dkeys, p->W_m, io.dfm, B * M, d->C, D, D, D, d->C);
    g1.add_colsum(L.dg_all, gr->b, 4 * D, rows_k, 4 * D);
    g1.add_colsum(L.dlogits, gr->b_o, V, Tp * B, pl.ldl);
    if (d->method == 0) {      // pgrad rows are [v | ln_g | ln_b | tau]: column sums over the rows
      const float* pg = pl.persist_b ? L.pgrad4 : L.pgrad;
      const int pr = pl.persist_b ? 4 * B : Tp * B, ldp = 3 * D + 1;
      g1.add_colsum(pg, gr->v, D, pr, ldp);
      g1.add_colsum(pg + D, gr->ln_g, D, pr, ldp);
      g1.add_colsum(pg + 2 * D, gr->ln_b, D, pr, ldp);
      g1.add_colsum(pg + 3 * D, gr->tau, 1, pr, ldp);
    }
    GemmGroupRun& gi = init_step ? g2 : g1;                       // d W_init (d im_embed) waits for d x_init of the first launch
    if (init_step) {
      ComicGemmProb* q = g1.add(COMIC_GG_NT, dg_init, p->K, L.dx_init, B, EA, 4 * D, 4 * D, 4 * D, EA);
      if (pl.drop_in) { q->mask = io.mask_init_in; q->ld_mask = EA; q->keep = d->keep_in; }
    }
    dx_im = init_step ? L.dx_init : L.dh;
    n_init = init_step ? EA : D;
    gi.add(COMIC_GG_TN, io.im_embed, dx_im, gr->W_init, d->Cg, n_init, B, d->Cg, n_init, n_init);
    if (io.dim_embed) gi.add(COMIC_GG_NT, dx_im, p->W_init, io.dim_embed, B, d->Cg, n_init, n_init, n_init, d->Cg);
    if (d->fm_projection == 1 && io.dfm) {
      ComicGemmProb* q = g2.add(COMIC_GG_NT, L.dvalues_buf, p->W_v, io.dfm, B * M, d->C, D, D, D, d->C);
      q->beta = 1.f;
    }
    RC(g1.run(L.gg_slab(), L.gg_slab_cap(), L.gg_tickets(), st));
    RC(comic_embed_bwd_set(L.in_tb, L.demb, gr->emb, Tp * B, E, V, st));
    RC(g2.run(L.gg_slab(), L.gg_slab_cap(), L.gg_tickets(), st));
    if (d->fm_projection == 0 && io.dfm) RC(comic_axpy(io.dfm, L.dvalues_buf, 1.f, (int64_t)B * M * Cv, (void*)st));
    return 0;
  }
  // ---- ... or on two lanes (side_lane).  Lane B: output projection, embedding, query layer, memory projections, attention
  // parameters; lane A (the caller's stream): output bias, cell kernel(s) and bias(es), then the rnn init
  int weight_grads_lanes() {
    LaneScope glane(pl.lane, st, L.splitk_b);
    RC(glane.rc);
    hipStream_t sb = glane.lane();
    RC(gemm_big(L.y_all, L.dlogits, gr->W_o, nullptr, D, V, Tp * B, D, V, V, 1, 0, 0.f, sb));
    if (pl.persist_b) {   // the embedding third of d gates * K^T, all steps at once, and its input dropout
      RC(gemm_big(L.dg_all, p->K, L.demb, nullptr, Tp * B, E, 4 * D, 4 * D, 4 * D, E, 0, 1, 0.f, sb));
      if (pl.drop_in) RC(comic_dropout_rows(L.demb, io.mask_in, d->keep_in, (long)Tp * B, E, EA, sb));
    }
    RC(fill(gr->emb, 0.f, (long)V * E, sb));
    RC(comic_embed_bwd(L.in_tb, L.demb, gr->emb, Tp * B, E, V, (void*)sb));
    RC(gemm_big(L.y_all, L.dq_all, gr->W_q, nullptr, D, D, Tp * B, D, D, D, 1, 0, 0.f, sb));
    RC(gemm_big(io.fm, L.dkeys, gr->W_m, nullptr, d->C, D, B * M, d->C, D, D, 1, 0, 0.f, sb));
    if (io.dfm) RC(gemm_big(L.dkeys, p->W_m, io.dfm, nullptr, B * M, d->C, D, D, D, d->C, 0, 1, 0.f, sb));
    if (d->fm_projection == 1) {
      RC(gemm_big(io.fm, L.dvalues_buf, gr->W_v, nullptr, d->C, D, B * M, d->C, D, D, 1, 0, 0.f, sb));
      if (io.dfm) RC(gemm_big(L.dvalues_buf, p->W_v, io.dfm, nullptr, B * M, d->C, D, D, D, d->C, 0, 1, 1.f, sb));
    } else if (d->fm_projection == 0 && io.dfm) {
      RC(comic_axpy(io.dfm, L.dvalues_buf, 1.f, (int64_t)B * M * Cv, (void*)sb));
    }
    if (d->method == 0) {        // pgrad rows are [v | ln_g | ln_b | tau]: column sums over the batch, then scatter
      float* tmp = L.pgrad_sum();
      RC(comic_colsum_ws(pl.persist_b ? L.pgrad4 : L.pgrad, tmp, pl.persist_b ? 4 * B : Tp * B, 3 * D + 1, 0.f, (float*)g_splitk_ws, sb));
      hipLaunchKernelGGL(scatter_pgrad_kernel, dim3(cdiv(D, 256)), dim3(256), 0, sb, (const float*)tmp, gr->v, gr->ln_g, gr->ln_b,
                         gr->tau, D);
    }
    glane.main_ws();
    RC(comic_colsum_ws(L.dlogits, gr->b_o, Tp * B, V, 0.f, (float*)g_splitk_ws, st));
    if (cell == COMIC_CELL_GRU) {
      RC(gemm_big(L.xh_all, L.dg_all, gr->K, nullptr, Wd, 2 * D, Tp * B, Wd, 4 * D, 2 * D, 1, 0, 0.f, st));
      RC(gemm_big(L.xh2_all, L.dg_all + 2 * D, gr->K_c, nullptr, Wd, D, Tp * B, Wd, 4 * D, D, 1, 0, 0.f, st));
      RC(comic_colsum_ws(L.dg_all, L.cell_tmp, Tp * B, 4 * D, 0.f, (float*)g_splitk_ws, st));
      COMIC_REQUIRE(hipMemcpyAsync(gr->b, L.cell_tmp, sizeof(float) * 2 * D, hipMemcpyDeviceToDevice, st) == hipSuccess &&
                        hipMemcpyAsync(gr->b_c, L.cell_tmp + 2 * D, sizeof(float) * D, hipMemcpyDeviceToDevice, st) == hipSuccess,
                    "train_step: bias gradient copy");
    } else {
      RC(gemm_big(L.xh_all, L.dg_all, gr->K, nullptr, Wd, 4 * D, Tp * B, Wd, 4 * D, 4 * D, 1, 0, 0.f, st));
      if (cell == COMIC_CELL_LSTM) RC(comic_colsum_ws(L.dg_all, gr->b, Tp * B, 4 * D, 0.f, (float*)g_splitk_ws, st));
    }
    RC(init_step_bwd());
    if (cell == COMIC_CELL_LN_LSTM) {           // LayerNorm gains / shifts: column sums of the per-row gradient rows
      const int rows = Tp * B + (d->init_method == 1 ? 0 : B);      // (the init step wrote its rows behind step Tp - 1's)
      RC(comic_colsum_ws(L.lnpg, L.cell_tmp, rows, 10 * D, 0.f, (float*)g_splitk_ws, st));
      RC(comic_ln_lstm_scatter(L.cell_tmp, gr->cell_ln, D, 0.f, st));
    }
    RC(gemm_big(io.im_embed, dx_im, gr->W_init, nullptr, d->Cg, n_init, B, d->Cg, n_init, n_init, 1, 0, 0.f, st));
    if (io.dim_embed) RC(gemm(dx_im, p->W_init, io.dim_embed, nullptr, B, d->Cg, n_init, n_init, n_init, d->Cg, 0, 1, 0.f, st));
    return glane.join();
  }

  // The rnn init step's backward (lane form; it accumulates into the cell's weight gradients): each cell's own launches
  // leave the init step's d pre-activations in ib.g, one tail turns them into d x_init = drop'(ib.g * K^T) [B][E+A]
  int init_step_bwd() {
    const InitBufs& ib = L.ib;
    dx_im = L.dh;
    n_init = D;
    if (d->init_method == 1) return 0;
    if (cell == COMIC_CELL_LN_LSTM) {
      RC(comic_ln_lstm_bwd(ib.gates, ib.lnx, ib.lnr, p->cell_ln, nullptr, ib.c_new, nullptr, nullptr, 0, nullptr, 1.f, nullptr, 0,
                           L.dc, L.dh, ib.g, L.lnpg + (size_t)Tp * B * 10 * D, B, D, st));
      RC(gemm(ib.xh, ib.g, gr->K, nullptr, EA, 4 * D, B, EA, 4 * D, 4 * D, 1, 0, 1.f, st));
    } else if (cell == COMIC_CELL_GRU) {        // zero state: d r_pre = 0
      RC(fill(ib.g, 0.f, (long)B * 4 * D, st));
      RC(comic_gru_bwd1(nullptr, nullptr, 0, nullptr, 1.f, nullptr, 0, L.dh, ib.gates, 4 * D, ib.gates + 2 * D, 4 * D, nullptr,
                        ib.g, 4 * D, B, D, st));
      RC(gemm(ib.xh, ib.g, gr->K, nullptr, EA, 2 * D, B, EA, 4 * D, 2 * D, 1, 0, 1.f, st));
      RC(gemm(ib.xh, ib.g + 2 * D, gr->K_c, nullptr, EA, D, B, EA, 4 * D, D, 1, 0, 1.f, st));
      RC(comic_colsum(ib.g, L.cell_tmp, B, 4 * D, 0.f, (void*)st));
      RC(comic_axpy(gr->b, L.cell_tmp, 1.f, 2 * D, (void*)st));
      RC(comic_axpy(gr->b_c, L.cell_tmp + 2 * D, 1.f, D, (void*)st));
    } else {
      RC(comic_lstm_gates_bwd(ib.gates, nullptr, ib.c_new, nullptr, nullptr, 1.f, nullptr, 0, L.dc, L.dh, ib.g, B, D, (void*)st));
      RC(gemm(ib.xh, ib.g, gr->K, nullptr, EA, 4 * D, B, EA, 4 * D, 4 * D, 1, 0, 1.f, st));
      RC(comic_colsum(ib.g, gr->b, B, 4 * D, 1.f, (void*)st));
    }
    if (cell == COMIC_CELL_GRU) {               // the gates' and the candidate's kernels
      RC(gemm(ib.g, p->K, L.dx_init, nullptr, B, EA, 2 * D, 4 * D, 2 * D, EA, 0, 1, 0.f, st));
      RC(gemm(ib.g + 2 * D, p->K_c, L.dx_init, nullptr, B, EA, D, 4 * D, D, EA, 0, 1, 1.f, st));
    } else {
      RC(gemm(ib.g, p->K, L.dx_init, nullptr, B, EA, 4 * D, 4 * D, 4 * D, EA, 0, 1, 0.f, st));
    }
    if (pl.drop_in) RC(comic_dropout_apply(L.dx_init, io.mask_init_in, d->keep_in, L.dx_init, (int64_t)B * EA, (void*)st));
    dx_im = L.dx_init;
    n_init = EA;
    return 0;
  }

  // ---- end-of-step gate: a persistent loop that timed out leaves garbage everywhere -- NaN losses and zero gradients (no
  // host check needed for the optimiser step that follows to be harmless; the host raises at its next look at the loss)
  int gate() {
    ComicGateRanges gr_{};
    int k = 0;
    auto add = [&](float* ptr, long n) {
      if (ptr && n > 0 && k < 16) { gr_.p[k] = ptr; gr_.n[k] = n; ++k; }
    };
    add(gr->W_init, (long)d->Cg * n_init); add(gr->K, (long)Wd * 4 * D); add(gr->b, 4L * D);      // (LSTM only: persist)
    add(gr->W_m, (long)d->C * D);
    if (d->fm_projection == 1) add(gr->W_v, (long)d->C * D);
    add(gr->W_q, (long)D * D);
    if (d->method == 0) { add(gr->v, D); add(gr->ln_g, D); add(gr->ln_b, D); add(gr->tau, 1); }
    if (d->context_layer) add(gr->W_a, (long)Cv * D);
    add(gr->W_o, (long)D * V); add(gr->b_o, V); add(gr->emb, (long)V * E);
    add(io.dfm, (long)B * M * d->C); add(io.dim_embed, (long)B * d->Cg);
    // COMIC_DEC_INJECT_TIMEOUT, fault injection for the tests of this gate: THIS call behaves as if one of its loops' bounded
    // waits had expired (the error word raised by hand)
    if (d->flags & COMIC_DEC_INJECT_TIMEOUT)
      COMIC_REQUIRE(hipMemsetAsync(L.persist_sync, 0xFF, sizeof(unsigned), st) == hipSuccess, "train_step: memset");
    return comic_persist_gate(L.persist_sync, io.loss_rows, io.map_loss, gr_, gr->status, p->status, st);
  }

  int run() {
    RC(validate_and_plan());
    if (pl.persist && pl.do_fwd) RC(prologue());
    if (pl.do_fwd) {
      RC(pl.grp ? forward_setup_grouped() : forward_setup_lanes());
      RC(operand_rows());
      RC(pl.persist ? forward_persistent() : forward_steps());
      if (pl.score) return score_tail();
      RC(logits());
    }
    if (!pl.do_bwd) {
      COMIC_LAUNCH_CHECK("train_step (forward phase)");
      return 0;
    }
    RC(loss_and_padding());
    RC(backward_prepare());
    RC(pl.persist_b ? backward_persistent() : backward_steps());
    RC(pl.grp ? weight_grads_grouped() : weight_grads_lanes());
    if (pl.persist) RC(gate());
    COMIC_LAUNCH_CHECK("train_step");
    return 0;
  }
};

int teacher_forced_step(const comic_decoder_desc* d, const comic_decoder_params* p, const comic_decoder_params* gr,
                        const StepIO& io, void* stream) {
  RC(check_desc(d));
  FlagScope flag_scope__(d);
  TeacherForcedStep step{d, p, gr, io, (hipStream_t)stream};
  return step.run();
}

// Scoring: dropout off, both phases' flags and the fault injection of the training step cleared
comic_decoder_desc score_desc(const comic_decoder_desc* d) {
  comic_decoder_desc s = *d;
  s.keep_in = s.keep_out = s.keep_alpha = 1.f;
  s.flags &= ~(uint32_t)(COMIC_DEC_PHASE_FWD | COMIC_DEC_PHASE_BWD | COMIC_DEC_INJECT_TIMEOUT);
  return s;
}

}  // namespace

extern "C" int64_t comic_decoder_train_workspace(const comic_decoder_desc* d, int B, int T) {
  if (!d) return -1;
  TrainLayout L;
  L.carve(d, B, T, TF_TRAIN, false, nullptr, 0);
  return (int64_t)L.bytes;
}

extern "C" int comic_decoder_train_step_soft(const comic_decoder_desc* d, const comic_decoder_params* p,
                                             const comic_decoder_params* gr, const float* fm, const float* im_embed,
                                             const int32_t* inputs_bt, const int32_t* targets_bt, const float* wmask_bt,
                                             const float* coef_bt, const int32_t* lens, int B, int T, int Tp,
                                             const float* mask_init_in, const float* mask_in, const float* mask_out,
                                             const float* mask_alpha, float* logits_tb, int32_t* ids_tb, float* attn_hist,
                                             float* loss_rows, float* map_loss, float* dfm, float* dim_embed,
                                             void* workspace, int64_t workspace_bytes, void* stream,
                                             const comic_soft_targets* soft) {
  if (soft) {           // refused before anything is launched
    COMIC_REQUIRE(d, "train_step_soft: null descriptor");
    COMIC_REQUIRE(soft->smoothing >= 0.f && soft->smoothing < 1.f, "train_step_soft: smoothing %g outside [0, 1)",
                  (double)soft->smoothing);
    COMIC_REQUIRE(soft->teacher_weight >= 0.f && soft->teacher_weight <= 1.f, "train_step_soft: teacher_weight %g outside [0, 1]",
                  (double)soft->teacher_weight);
    COMIC_REQUIRE(soft->smoothing + soft->teacher_weight <= 1.f, "train_step_soft: smoothing + teacher_weight = %g exceeds 1",
                  (double)(soft->smoothing + soft->teacher_weight));
    if (soft->teacher_weight > 0.f) {
      COMIC_REQUIRE(soft->ids_tbk && soft->probs_tbk, "train_step_soft: teacher_weight %g without a teacher table",
                    (double)soft->teacher_weight);
      COMIC_REQUIRE(soft->K >= 1 && soft->K <= COMIC_SOFT_MAX_K && soft->K <= d->V,
                    "train_step_soft: K %d outside [1, min(%d, V)]", soft->K, COMIC_SOFT_MAX_K);
    }
  }
  StepIO io{};
  io.soft = soft;
  io.fm = fm; io.im_embed = im_embed; io.inputs_bt = inputs_bt; io.targets_bt = targets_bt; io.wmask_bt = wmask_bt;
  io.coef_bt = coef_bt; io.lens = lens; io.B = B; io.T = T; io.Tp = Tp;
  io.mask_init_in = mask_init_in; io.mask_in = mask_in; io.mask_out = mask_out; io.mask_alpha = mask_alpha;
  io.logits_tb = logits_tb; io.ids_tb = ids_tb; io.attn_hist = attn_hist; io.loss_rows = loss_rows; io.map_loss = map_loss;
  io.dfm = dfm; io.dim_embed = dim_embed; io.workspace = workspace; io.workspace_bytes = workspace_bytes;
  return teacher_forced_step(d, p, gr, io, stream);
}

extern "C" int comic_decoder_train_step(const comic_decoder_desc* d, const comic_decoder_params* p,
                                        const comic_decoder_params* gr, const float* fm, const float* im_embed,
                                        const int32_t* inputs_bt, const int32_t* targets_bt, const float* wmask_bt,
                                        const float* coef_bt, const int32_t* lens, int B, int T, int Tp,
                                        const float* mask_init_in, const float* mask_in, const float* mask_out,
                                        const float* mask_alpha, float* logits_tb, int32_t* ids_tb, float* attn_hist,
                                        float* loss_rows, float* map_loss, float* dfm, float* dim_embed,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
  return comic_decoder_train_step_soft(d, p, gr, fm, im_embed, inputs_bt, targets_bt, wmask_bt, coef_bt, lens, B, T, Tp,
                                       mask_init_in, mask_in, mask_out, mask_alpha, logits_tb, ids_tb, attn_hist, loss_rows,
                                       map_loss, dfm, dim_embed, workspace, workspace_bytes, stream, nullptr);
}

// the scoring layout (the caller takes no alignment history: the workspace holds it), with the flags that select the
// projection's form latched as in the call itself
extern "C" int64_t comic_decoder_score_workspace(const comic_decoder_desc* d, int B, int T) {
  if (!d || B <= 0 || T <= 0) return -1;
  const comic_decoder_desc s = score_desc(d);
  if (check_desc(&s)) return -1;
  FlagScope flag_scope__(&s);
  TrainLayout L;
  L.carve(&s, B, T, TF_SCORE, true, nullptr, 0);
  return (int64_t)L.bytes;
}

extern "C" int comic_decoder_score(const comic_decoder_desc* d, const comic_decoder_params* p, const float* fm,
                                   const float* im_embed, const int32_t* inputs_bt, const int32_t* targets_bt,
                                   const float* wmask_bt, const int32_t* lens, int B, int T, int Tp, float* token_logp_tb,
                                   float* caption_logp, float* attn_hist, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
  COMIC_REQUIRE(d, "score: null descriptor");
  const comic_decoder_desc s = score_desc(d);
  StepIO io{};
  io.fm = fm; io.im_embed = im_embed; io.inputs_bt = inputs_bt; io.targets_bt = targets_bt; io.wmask_bt = wmask_bt;
  io.lens = lens; io.B = B; io.T = T; io.Tp = Tp; io.attn_hist = attn_hist;
  io.score = true; io.token_logp_tb = token_logp_tb; io.caption_logp = caption_logp; io.workspace = workspace; io.workspace_bytes = workspace_bytes;
  return teacher_forced_step(&s, p, nullptr, io, stream);
}

// columns of the W_o scratch: V rounded up to whole chunks of any of its packed forms (128, 112 or 64 columns)
static inline long wo_pad_cols(long V) { return (V + 127) / 128 * 128 + 128; }
constexpr int kBeamCntSteps = 4096;       // decode steps the in-kernel completion counters of the beam step cover

namespace {
// Workspace of the decode loops.  carve_infer is the ONE definition of its blocks: comic_decoder_infer_workspace runs it over a
// null base, greedy / sampling / beam search over the caller's buffer.
struct InferBufs {
  float *fm_t, *im_t, *keys, *values_buf;
  InitBufs ib;
  StepBufs sb;
  float *c[2], *h[2], *att[2], *x, *logits, *log_probs, *gtmp, *kpanel, *wo_pad, *kfrag, *xfrag, *wqfrag, *yfrag;
  unsigned long long* beam_cnt = nullptr;
  int32_t *ids, *parents;
  float *p_xh = nullptr, *p_y = nullptr, *p_q = nullptr, *p_argp = nullptr;   // persistent greedy loop (rows <= 64)
  unsigned* p_sync = nullptr;
  void* splitk;              // split-K partials (the executor points g_splitk_ws at it)
  size_t bytes;
  bool ok;
};
// max_steps > 0: the hand-off buffers of the persistent greedy loop (rows <= 64), [max_steps] rows each, behind everything else
InferBufs carve_infer(const comic_decoder_desc* d, int rows, void* ws, int64_t bytes, int max_steps) {
  Bump w(ws, (size_t)bytes);
  const long D = d->D, E = d->E, A = d->A, V = d->V, M = d->M, H = d->H, Cv = d->Cv, Wd = E + A + D, R = rows;
  InferBufs b;
  b.fm_t = w.take<float>(R * M * d->C); b.im_t = w.take<float>(R * d->Cg);
  b.keys = w.take<float>(R * M * D); b.values_buf = w.take<float>(R * M * D);
  b.ib.x = w.take<float>(R * (E + A)); b.ib.xh = w.take<float>(R * (E + A));
  b.ib.g = w.take<float>(R * 4 * D); b.ib.gates = w.take<float>(R * 4 * D); b.ib.c_new = w.take<float>(R * D);
  b.sb.xh = w.take<float>(R * Wd); b.sb.g = w.take<float>(R * 4 * D); b.sb.y = w.take<float>(R * D);
  b.sb.q = w.take<float>(R * D); b.sb.alpha = w.take<float>(R * H * M); b.sb.ctx = w.take<float>(R * Cv);
  b.c[0] = w.take<float>(R * D); b.c[1] = w.take<float>(R * D);
  b.h[0] = w.take<float>(R * D); b.h[1] = w.take<float>(R * D);
  b.sb.att2 = w.take<float>(R * D);
  b.att[0] = w.take<float>(R * A); b.att[1] = w.take<float>(R * A);
  b.x = w.take<float>(R * E); b.logits = w.take<float>(R * V);
  b.ids = w.take<int32_t>(R); b.log_probs = w.take<float>(R); b.parents = w.take<int32_t>(R);
  b.gtmp = w.take<float>(R * (2 * D + A));
  b.splitk = w.take<char>(kSplitKBytes);
  b.kpanel = w.take<float>(comic_lstm_panel_floats(d->D, d->E + d->A + d->D, 0));
  b.wo_pad = w.take<float>((D + 1) * wo_pad_cols(V));      // W_o with 16-byte aligned rows / packed hi-lo fragments + bias
  b.kfrag = w.take<float>(comic_lstm_stream_kfrag_floats(d->D, (int)Wd)); b.xfrag = w.take<float>(comic_lstm_stream_xfrag_floats(rows, (int)Wd));
  b.wqfrag = w.take<float>(comic_stream_gemm_wfrag_floats(d->D, d->D)); b.yfrag = w.take<float>(comic_lstm_stream_xfrag_floats(rows, d->D));
  b.beam_cnt = w.take<unsigned long long>(kBeamCntSteps);
  if (d->cell == COMIC_CELL_GRU) b.sb.xh2 = w.take<float>(R * Wd);
  if (rows <= 64 && max_steps > 0) {
    const long S = max_steps;
    b.p_xh = w.take<float>(S * R * Wd); b.p_y = w.take<float>(S * R * D); b.p_q = w.take<float>(S * R * D);
    b.p_argp = w.take<float>(S * R * 132);
    b.p_sync = w.take<unsigned>(kPersistSyncWords);
  }
  b.bytes = w.off;
  b.ok = w.ok;
  return b;
}

// The output projection is streamed once per decode step.  Its rows ([D][V], TensorFlow layout) are 16-byte aligned
// only when V % 4 == 0 (V = 25 599 for the word vocabulary, 258 for radix-256): a copy with padded rows lets the
// product kernels use 16-byte loads (4x fewer load instructions on the dominant operand).  Returns the matrix and
// its leading dimension to use for this call.
const float* aligned_w_o(const comic_decoder_desc* d, const comic_decoder_params* p, float* pad, int* ldb,
                         hipStream_t st) {
  const int V = d->V, Vp = (V + 3) / 4 * 4;
  if (V == Vp || !pad) {
    *ldb = V;
    return p->W_o;
  }
  const long n = (long)d->D * Vp;
  hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, p->W_o, pad, V, Vp, n);
  *ldb = Vp;
  return pad;
}
}  // namespace

// The size covers the greedy loop's hand-off buffers whenever rows <= 64, for one step at the least: beam search asks with
// the same entry and carves without them (max_steps 0), its blocks sit in front of them.
extern "C" int64_t comic_decoder_infer_workspace(const comic_decoder_desc* d, int rows, int max_steps) {
  if (!d) return -1;
  return (int64_t)carve_infer(d, rows, nullptr, 0, std::max(1, max_steps)).bytes;
}

int comic_argmax_rows_noise(const float* x, const float* noise, int32_t* idx, int rows, int V, hipStream_t st);

// greedy (gumbel_tb null) or sampled (gumbel_tb [max_steps][B][V]: ids = argmax(logits + noise)) decode loop
static int decoder_search(const comic_decoder_desc* d, const comic_decoder_params* p, const float* fm,
                          const float* im_embed, int B, int max_steps, const float* gumbel_tb, int32_t* ids_tb,
                          float* logits_tb, float* attn_hist, int32_t* first_eos, void* workspace,
                          int64_t workspace_bytes, void* stream) {
  RC(check_desc(d));
  FlagScope flag_scope__(d);
  COMIC_REQUIRE(p && fm && im_embed && ids_tb && attn_hist && first_eos && workspace, "greedy: null pointer");
  COMIC_REQUIRE(B > 0 && max_steps > 0, "greedy: bad shape");
  COMIC_REQUIRE(workspace_bytes >= comic_decoder_infer_workspace(d, B, max_steps), "greedy: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  InferBufs ws = carve_infer(d, B, workspace, workspace_bytes, max_steps);
  COMIC_REQUIRE(ws.ok, "greedy: workspace overflow");
  g_splitk_ws = ws.splitk;
  const int D = d->D, E = d->E, A = d->A, V = d->V, M = d->M, H = d->H, Cv = d->Cv;
  const comic_attn_desc ad = attn_desc(d, B);
  const float* values = nullptr;
  RC(memory_projections(d, p, fm, B, ws.keys, ws.values_buf, &values, st));
  RC(rnn_init_fwd(d, p, im_embed, B, nullptr, ws.ib, ws.c[0], ws.h[0], st));
  RC(fill(ws.att[0], 0.f, (long)B * A, st));
  hipLaunchKernelGGL(fill_i32_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, ws.ids, d->start_id, (long)B);
  hipLaunchKernelGGL(fill_i32_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, first_eos, max_steps, (long)B);
  int32_t* steps_done = ws.parents;        // beam-only buffer: its first word is this loop's end marker
  hipLaunchKernelGGL(fill_i32_kernel, dim3(1), dim3(64), 0, st, steps_done, max_steps, 1L);
  COMIC_LAUNCH_CHECK("greedy init");
  const bool fused = fused_step_enabled() && comic_fused_step_supported(D, E + A + D);
  if (fused) RC(comic_pack_lstm_panels(p->K, ws.kpanel, nullptr, D, E + A + D, st));
  // the whole loop as one persistent launch (decoder_persist.hip, GREEDY) when the shape allows it
  g_greedy_path = 0;
  if (!gumbel_tb && fused && persist_enabled() && ws.p_xh &&
      comic_persist_greedy_supported(B, D, E, A, M, H, Cv, V, d->method, d->context_layer, ad.tied) &&
      comic_persist_fits_device(B)) {
    const int Wd = E + A + D;
    ComicPersistRanges pr{};
    pr.p[0] = ws.p_xh; pr.n[0] = (long)max_steps * B * Wd;
    pr.p[1] = ws.p_y; pr.n[1] = (long)max_steps * B * D;
    pr.p[2] = ws.p_q; pr.n[2] = (long)max_steps * B * D;
    pr.p[3] = ws.p_argp; pr.n[3] = (long)max_steps * B * 132;
    RC(comic_persist_prepare(pr, ws.p_sync, kPersistSyncWords, st));
    // step 0 operand: att = 0, h = h0 (the x third comes from the embedding table inside the loop)
    {
      const long n = (long)B * A + (long)B * D;
      hipLaunchKernelGGL(embed_step0_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, p->emb,
                         (const int32_t*)nullptr, (int32_t*)nullptr, (const float*)nullptr, 1.f, ws.p_xh, ws.att[0], ws.h[0],
                         0, B, 0, E, A, D, V, (float*)nullptr, (const float*)nullptr, (float*)nullptr, (float*)nullptr,
                         (float*)nullptr, (float*)nullptr);
      COMIC_LAUNCH_CHECK("greedy step0");
    }
    ComicPersistFwdArgs pa{};
    pa.K_panel = ws.kpanel; pa.bias = p->b; pa.W_q = p->W_q; pa.keys = ws.keys; pa.values = values;
    pa.ln_g = p->ln_g; pa.ln_b = p->ln_b; pa.v = p->v; pa.tau = p->tau;
    pa.keep_in = pa.keep_out = pa.keep_alpha = 1.f;
    pa.xh_all = ws.p_xh; pa.y_all = ws.p_y; pa.q_all = ws.p_q; pa.cs = ws.c[0]; pa.hs = ws.h[0];
    pa.attn_hist = attn_hist; pa.sync = ws.p_sync;
    pa.B = B; pa.D = D; pa.E = E; pa.Wd = Wd; pa.M = M; pa.H = H; pa.Tp = max_steps;
    pa.method = d->method; pa.prob = d->prob; pa.tied = ad.tied;
    pa.grp0 = 0; pa.n_groups = (B + 15) / 16;
    pa.greedy = 1; pa.emb = p->emb; pa.W_o = p->W_o; pa.b_o = p->b_o; pa.V = V; pa.ld_wo = V;
    pa.start_id = d->start_id; pa.end_id = d->end_id;
    pa.argp = ws.p_argp; pa.ids_tb = ids_tb; pa.first_eos = first_eos; pa.logits_tb = logits_tb;
    RC(comic_persist_fwd_launch(pa, st));
    RC(comic_persist_check_greedy(ws.p_sync, first_eos, st));
    g_greedy_path = 1;
    return 0;
  }
  int ld_wo = V;
  const float* w_o = aligned_w_o(d, p, ws.wo_pad, &ld_wo, st);
  struct StopScope {          // whatever way this call returns, no later launch sees the flag
    ~StopScope() { g_comic_stop = ComicStop(); }
  } stop_scope;
  for (int t = 0; t < max_steps; ++t) {
    if (fused) {              // the step's kernels return at once when the loop ended earlier (fused path only)
      g_comic_stop.p = steps_done;
      g_comic_stop.t = t;
    }
    const int cur = t & 1, nxt = cur ^ 1;
    ws.sb.c2 = ws.c[nxt];
    ws.sb.h2 = ws.h[nxt];
    float* att_next = ws.att[nxt];
    StepBufs sb = ws.sb;
    if (!d->context_layer) sb.ctx = att_next;  // context written straight into the next attention state
    else sb.att2 = att_next;
    // the ids of step t-1 are read where argmax wrote them (ids_tb), no copy
    const int32_t* ids_in = t == 0 ? ws.ids : ids_tb + (size_t)(t - 1) * B;
    if (fused) {
      RC(infer_step_fused(d, p, ad, ws.keys, values, ws.kpanel, ids_in, nullptr, 1, ws.c[cur], ws.h[cur], ws.att[cur],
                          sb, ws.gtmp, attn_hist + (size_t)t * B * H * M, B, st));
    } else {
      RC(comic_embed_fwd(p->emb, ids_in, ws.x, B, E, V, (void*)st));
      RC(infer_step(d, p, ad, ws.keys, values, ws.x, ws.c[cur], ws.h[cur], ws.att[cur], sb,
                    attn_hist + (size_t)t * B * H * M, B, st));
    }
    float* lg = logits_tb ? logits_tb + (size_t)t * B * V : ws.logits;
    RC(gemm(sb.y, w_o, lg, p->b_o, B, V, D, D, ld_wo, V, 0, 0, 0.f, st));
    int32_t* ids_out = ids_tb + (size_t)t * B;
    RC(comic_argmax_rows_noise(lg, gumbel_tb ? gumbel_tb + (size_t)t * B * V : nullptr, ids_out, B, V, st));
    hipLaunchKernelGGL(eos_track_done_kernel, dim3(1), dim3(256), 0, st, (const int32_t*)ids_out, first_eos, t,
                       d->end_id, B, steps_done, max_steps);
    COMIC_LAUNCH_CHECK("eos_track");
  }
  return 0;
}

extern "C" int comic_decoder_greedy(const comic_decoder_desc* d, const comic_decoder_params* p, const float* fm,
                                    const float* im_embed, int B, int max_steps, int32_t* ids_tb, float* logits_tb,
                                    float* attn_hist, int32_t* first_eos, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
  return decoder_search(d, p, fm, im_embed, B, max_steps, nullptr, ids_tb, logits_tb, attn_hist, first_eos, workspace,
                        workspace_bytes, stream);
}
extern "C" int comic_decoder_sample(const comic_decoder_desc* d, const comic_decoder_params* p, const float* fm,
                                    const float* im_embed, int B, int max_steps, const float* gumbel_tb, int32_t* ids_tb,
                                    float* logits_tb, float* attn_hist, int32_t* first_eos, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  COMIC_REQUIRE(gumbel_tb, "sample: null noise");
  return decoder_search(d, p, fm, im_embed, B, max_steps, gumbel_tb, ids_tb, logits_tb, attn_hist, first_eos, workspace,
                        workspace_bytes, stream);
}

// ---- one beam step from the decoder outputs, as an operator (C-ABI) -----------------------------------------------------
// logits = y W_o + b_o, log_softmax, _mask_probs, top-k over beam x V, bookkeeping ([TF-1.9] _beam_search_step as used by
// rnn_decoder_beam_search, ops_rnn.py:49-112) with the kernels comic_decoder_beam picks for the shape: the streaming
// projection + per-chunk top-k + merge (V >= 4096, D % 128 == 0), the register-resident small step (V <= 1024), the GEMM +
// comic_beam_step chain otherwise.  The same state arrays as comic_beam_step.
static int64_t beam_dense_region(int B, int W, int D, int V) {        // floats: logits / partials
  const int64_t R = (int64_t)B * W;
  return std::max<int64_t>(R * V, comic_beam_logits_supported(D, V, (int)R, W) ? comic_beam_logits_partial_floats(D, V, (int)R, W, 1) : 0) + 64;
}
extern "C" int64_t comic_beam_step_dense_workspace(int B, int W, int D, int V) {
  if (B <= 0 || W <= 0 || D <= 0 || V <= 0) return -1;
  return ((int64_t)(D + 1) * wo_pad_cols(V) + beam_dense_region(B, W, D, V)) * 4 + kSplitKBytes + 4096;
}
// (prep: the NEXT step's operand rows through the parents just chosen, as the beam loop hands them to the streaming LSTM
// step -- comic_op_beam_step_prep; only the merge and the small step take it)
static int beam_step_dense_impl(const float* y, const float* W_o, const float* b_o, float* log_probs, int32_t* finished,
                                int64_t* lengths, int32_t* word_ids, int32_t* parent_ids, float* scores, int B, int W, int D,
                                int V, int end_id, const LstmPrepArgs* prep, void* workspace, int64_t workspace_bytes,
                                void* stream) {
  COMIC_REQUIRE(y && W_o && b_o && log_probs && finished && lengths && word_ids && parent_ids && scores && workspace,
                "beam_step_dense: null pointer");
  COMIC_REQUIRE(B > 0 && W > 0 && W <= 64 && D > 0 && V >= W, "beam_step_dense: bad shape");
  COMIC_REQUIRE(workspace_bytes >= comic_beam_step_dense_workspace(B, W, D, V), "beam_step_dense: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  Bump w(workspace, (size_t)workspace_bytes);
  float* wo = w.take<float>((D + 1) * wo_pad_cols(V));
  float* region = w.take<float>(beam_dense_region(B, W, D, V));
  void* splitk = w.take<char>(kSplitKBytes);
  int32_t* steps = w.take<int32_t>(16);
  unsigned long long* cnt = (unsigned long long*)w.take<int64_t>(16);
  COMIC_REQUIRE(w.ok, "beam_step_dense: workspace overflow");
  const int R = B * W;
  hipLaunchKernelGGL(fill_i32_kernel, dim3(1), dim3(64), 0, st, steps, 1, 1L);
  if (comic_beam_logits_supported(D, V, R, W)) {
    RC(comic_beam_pack_wo(W_o, b_o, V, wo, D, V, st));
    RC(comic_beam_logits_begin(region, B, W, V, 1, st));
    return comic_beam_logits_step(y, nullptr, wo, region, log_probs, finished, lengths, word_ids, parent_ids, scores, steps, 0, 1,
                                  B, W, D, V, end_id, prep, st);
  }
  COMIC_REQUIRE(!prep || comic_beam_step_small_supported(V, W),
                "beam_step_prep: neither the merge nor the small step serves this shape (D %d, V %d, beam %d)", D, V, W);
  RC(comic_gemm_bf16x3_impl(y, W_o, region, b_o, R, V, D, D, V, V, 0, 0, 1.f, 0.f, splitk, kSplitKBytes, st));
  if (comic_beam_step_small_supported(V, W)) {
    RC(comic_beam_counters_zero(cnt, 1, st));
    return comic_beam_step_small(region, nullptr, 1, V, 0, log_probs, finished, lengths, word_ids, parent_ids, scores, B, W, V,
                                 end_id, cnt, steps, 0, 1, prep, st);
  }
  return comic_beam_step_ws(region, log_probs, finished, lengths, word_ids, parent_ids, scores, B, W, V, end_id, 0.f, splitk,
                            kSplitKBytes, st);
}
extern "C" int comic_beam_step_dense(const float* y, const float* W_o, const float* b_o, float* log_probs, int32_t* finished,
                                     int64_t* lengths, int32_t* word_ids, int32_t* parent_ids, float* scores, int B, int W,
                                     int D, int V, int end_id, void* workspace, int64_t workspace_bytes, void* stream) {
  return beam_step_dense_impl(y, W_o, b_o, log_probs, finished, lengths, word_ids, parent_ids, scores, B, W, D, V, end_id,
                              nullptr, workspace, workspace_bytes, stream);
}

// ---- op-level entries of the decode loops' LSTM half step and of the operand hand-off behind the beam merge ----------------
// (include/comic_hip.h, "op-level entries"; tests only.)  comic_op_beam_step_prep: comic_beam_step_dense with the record the
// beam loop passes when the streaming LSTM step follows; x_frag: comic_lstm_stream_xfrag_floats(B W, E + A + D) floats,
// c_in [B W][D].  Workspace: comic_beam_step_dense_workspace.
extern "C" int comic_op_beam_step_prep(const float* y, const float* W_o, const float* b_o, float* log_probs, int32_t* finished,
                                       int64_t* lengths, int32_t* word_ids, int32_t* parent_ids, float* scores, int B, int W,
                                       int D, int V, int end_id, const float* table, const float* att, const float* h,
                                       const float* c, void* x_frag, float* c_in, int E, int A, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  COMIC_REQUIRE(table && att && h && c && x_frag && c_in, "beam_step_prep: null pointer");
  COMIC_REQUIRE(E > 0 && A > 0 && D > 0 && E % 8 == 0 && A % 8 == 0 && D % 8 == 0,
                "beam_step_prep: the operand thirds must be multiples of 8 (E %d, A %d, D %d)", E, A, D);
  const LstmPrepArgs prep{table, att, h, c, (uint4*)x_frag, c_in, E, A, D, V, (E + A + D + 31) / 32};
  return beam_step_dense_impl(y, W_o, b_o, log_probs, finished, lengths, word_ids, parent_ids, scores, B, W, D, V, end_id, &prep,
                              workspace, workspace_bytes, stream);
}

// comic_op_infer_lstm_step: infer_step_lstm on raw parameters.  stream = 0: infer_prep_kernel + comic_lstm_step_fused over
// the forward panel; stream = 1: comic_lstm_stream_pack once, then comic_lstm_stream_step (x_frag / y_frag:
// comic_lstm_stream_xfrag_floats(R, Wd) / (R, D) floats).  stop / stop_t: the decode loops' stop word for these launches.
static int64_t op_infer_lstm_carve(int R, int D, int E, int A, int stream, void* base, int64_t bytes, float** wpack, float** xh,
                                   void** part) {
  const int Wd = E + A + D;
  Bump w(base, (size_t)bytes);
  *wpack = w.take<float>(stream ? comic_lstm_stream_kfrag_floats(D, Wd) : comic_lstm_panel_floats(D, Wd, 0));
  *xh = w.take<float>(stream ? 0 : (size_t)R * Wd);
  *part = w.take<char>(stream ? comic_lstm_stream_part_bytes(D, Wd, R) : 0);
  return w.ok ? (int64_t)w.off : -1;
}
extern "C" int64_t comic_op_infer_lstm_step_workspace(int R, int D, int E, int A, int stream) {
  if (R <= 0 || D <= 0 || E <= 0 || A <= 0) return -1;
  float *a, *b;
  void* c;
  return op_infer_lstm_carve(R, D, E, A, stream, nullptr, 0, &a, &b, &c);
}
extern "C" int comic_op_infer_lstm_step(const float* table, const int32_t* ids, const int32_t* parent, int W,
                                        const float* att_src, const float* h_src, const float* c_src, const float* K,
                                        const float* bias, float* c_in, float* c2, float* h2, float* y, void* x_frag,
                                        void* y_frag, int R, int E, int A, int D, int V, int stream_lstm, const int32_t* stop,
                                        int stop_t, void* workspace, int64_t workspace_bytes, void* stream) {
  COMIC_REQUIRE(table && ids && att_src && h_src && c_src && K && c_in && c2 && h2 && y && workspace, "op_infer_lstm_step: null pointer");
  COMIC_REQUIRE(R > 0 && W > 0 && R % W == 0 && D > 0 && E > 0 && A > 0 && V > 0, "op_infer_lstm_step: bad shape");
  const int Wd = E + A + D;
  if (stream_lstm) {
    COMIC_REQUIRE(x_frag && y_frag, "op_infer_lstm_step: null fragment buffer");
    COMIC_REQUIRE(comic_lstm_stream_supported(D, E, A, R), "op_infer_lstm_step: the streaming step does not serve D %d, E %d, A %d, rows %d", D, E, A, R);
    COMIC_REQUIRE(comic_lstm_stream_part_bytes(D, Wd, R) <= kSplitKBytes, "op_infer_lstm_step: K-slice partials beyond the split-K scratch");
  } else {
    COMIC_REQUIRE(comic_fused_step_supported(D, Wd), "op_infer_lstm_step: the fused step does not serve D %d, Wd %d", D, Wd);
  }
  float *wpack, *xh;
  void* part;
  const int64_t need = op_infer_lstm_carve(R, D, E, A, stream_lstm, workspace, workspace_bytes, &wpack, &xh, &part);
  COMIC_REQUIRE(need >= 0, "op_infer_lstm_step: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  comic_decoder_desc d{};
  d.D = D; d.E = E; d.A = A; d.V = V;
  comic_decoder_params p{};
  p.emb = const_cast<float*>(table); p.b = const_cast<float*>(bias);      // read only by the step
  StepBufs sb{};
  sb.xh = xh; sb.y = y; sb.c2 = c2; sb.h2 = h2;
  StreamBufs sm{wpack, x_frag, y_frag, nullptr};
  if (stream_lstm) RC(comic_lstm_stream_pack(K, wpack, D, Wd, st));
  else RC(comic_pack_lstm_panels(K, wpack, nullptr, D, Wd, st));
  struct Scope {              // the stop word and the split-K scratch of this call only
    void* saved_ws = g_splitk_ws;
    ~Scope() {
      g_comic_stop = ComicStop();
      g_splitk_ws = saved_ws;
    }
  } scope;
  g_comic_stop.p = stop;
  g_comic_stop.t = stop_t;
  g_splitk_ws = part;
  return infer_step_lstm(&d, &p, wpack, ids, parent, W, c_src, h_src, att_src, sb, c_in, R, st, stream_lstm ? &sm : nullptr);
}

// ---- beam search: what a single decoder and every member of an ensemble share ---------------------------------------------
struct BeamMember {
  bool fused = false, stream_lstm = false;
  int mem_div = 1, ld_wo = 0, cur = 0;
  comic_attn_desc ad{};
  const float* values = nullptr;
  const float* w_o = nullptr;      // (with ld_wo) set by the loop that projects with the GEMM
  StreamBufs sm{};
};
// The member's state before step 0: tiled inputs, keys / values, initial c / h / attention, and its LSTM weights packed for
// the step kernel its shape selects.
static int beam_member_begin(const comic_decoder_desc* d, const comic_decoder_params* p, const float* fm, const float* im_embed,
                             int B, int W, InferBufs& ws, hipStream_t st, BeamMember& e) {
  const int R = B * W, D = d->D, E = d->E, A = d->A, M = d->M;
  // tile_batch BEFORE keys are computed (model_base.py:127-131).  The beams of an entry attend to the same memory: the
  // fused step's attention kernel reads row b / W of keys / values held ONCE per entry (same values as the tiled copy's)
  e.fused = fused_step_enabled() && comic_fused_step_supported(D, E + A + D);
  e.mem_div = e.fused ? W : 1;
  {
    const long n1 = (long)R * M * d->C, n2 = (long)R * d->Cg;
    if (e.mem_div == 1)
      hipLaunchKernelGGL(tile_rows_kernel, dim3((unsigned)cdiv64(n1, 256)), dim3(256), 0, st, fm, ws.fm_t, n1, W,
                         M * d->C);
    hipLaunchKernelGGL(tile_rows_kernel, dim3((unsigned)cdiv64(n2, 256)), dim3(256), 0, st, im_embed, ws.im_t, n2, W,
                       d->Cg);
    COMIC_LAUNCH_CHECK("tile_rows");
  }
  e.ad = attn_desc(d, R);
  if (e.mem_div == 1) RC(memory_projections(d, p, ws.fm_t, R, ws.keys, ws.values_buf, &e.values, st));
  else RC(memory_projections(d, p, fm, B, ws.keys, ws.values_buf, &e.values, st));
  RC(rnn_init_fwd(d, p, ws.im_t, R, nullptr, ws.ib, ws.c[0], ws.h[0], st));
  RC(fill(ws.att[0], 0.f, (long)R * A, st));
  e.stream_lstm = e.fused && lstm_stream_enabled() && comic_lstm_stream_supported(D, E, A, R) &&
                  comic_lstm_stream_part_bytes(D, E + A + D, R) <= kSplitKBytes;
  e.sm = StreamBufs{ws.kfrag, ws.xfrag, ws.yfrag, nullptr};
  if (e.stream_lstm) {
    RC(comic_lstm_stream_pack(p->K, ws.kfrag, D, E + A + D, st));
    if (comic_stream_gemm_supported(D, D, R) && comic_stream_gemm_part_bytes(D, D, R) <= kSplitKBytes) {
      RC(comic_stream_gemm_pack(p->W_q, ws.wqfrag, D, D, st));
      e.sm.wqfrag = ws.wqfrag;
    }
  } else if (e.fused) RC(comic_pack_lstm_panels(p->K, ws.kpanel, nullptr, D, E + A + D, st));
  return 0;
}
// Where a step writes: fused, the raw outputs ping-pong into c / h / att[nxt] and the NEXT step's operand prep gathers them
// through the parents chosen in between (no gather / copy / embedding kernels); unfused, they land in gtmp and the loop
// re-orders them itself.  *att_new is the step's new attention state in either form.
static StepBufs beam_step_bufs(const comic_decoder_desc* d, const InferBufs& ws, bool fused, int nxt, int R, float** att_new) {
  StepBufs sb = ws.sb;
  sb.c2 = fused ? ws.c[nxt] : ws.gtmp;
  sb.h2 = fused ? ws.h[nxt] : ws.gtmp + (size_t)R * d->D;
  *att_new = fused ? ws.att[nxt] : ws.gtmp + (size_t)2 * R * d->D;
  if (!d->context_layer) sb.ctx = *att_new;
  else sb.att2 = *att_new;
  return sb;
}

extern "C" int comic_decoder_beam(const comic_decoder_desc* d, const comic_decoder_params* p, const float* fm,
                                  const float* im_embed, int B, int W, int max_steps, int32_t* step_ids,
                                  int32_t* parent_ids, float* scores, int64_t* lengths, int32_t* finished,
                                  float* attn_hist, int32_t* steps_executed, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  RC(check_desc(d));
  FlagScope flag_scope__(d);
  COMIC_REQUIRE(p && fm && im_embed && step_ids && parent_ids && scores && lengths && finished && attn_hist &&
                    steps_executed && workspace,
                "beam: null pointer");
  COMIC_REQUIRE(B > 0 && W > 0 && W <= 64 && max_steps > 0, "beam: bad shape");
  const int R = B * W;
  COMIC_REQUIRE(workspace_bytes >= comic_decoder_infer_workspace(d, R, max_steps), "beam: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  InferBufs ws = carve_infer(d, R, workspace, workspace_bytes, 0);
  COMIC_REQUIRE(ws.ok, "beam: workspace overflow");
  g_splitk_ws = ws.splitk;
  const int D = d->D, E = d->E, A = d->A, V = d->V, M = d->M, H = d->H;
  // initial beam state: log_probs [0,-inf,...], finished [0,1,...], lengths 0
  hipLaunchKernelGGL(beam_init_kernel, dim3(cdiv(R, 256)), dim3(256), 0, st, ws.log_probs, finished, lengths, R, W);
  hipLaunchKernelGGL(fill_i32_kernel, dim3(cdiv(R, 256)), dim3(256), 0, st, ws.ids, d->start_id, (long)R);
  hipLaunchKernelGGL(fill_i32_kernel, dim3(1), dim3(64), 0, st, steps_executed, max_steps, 1L);
  COMIC_LAUNCH_CHECK("beam init");
  BeamMember mem;
  RC(beam_member_begin(d, p, fm, im_embed, B, W, ws, st, mem));
  const bool fused = mem.fused, stream_lstm = mem.stream_lstm;
  StreamBufs& sm = mem.sm;
  // large vocabularies: projection + per-chunk top-k as one streaming launch over a packed W_o (beam_logits.hip)
  // (a length penalty ranks by score, not by log probability: its step runs the one-workgroup-per-entry kernel)
  const float lpw = d->length_penalty_weight;
  const bool stream_logits = fused && lpw == 0.f && beam_logits_enabled() && comic_beam_logits_supported(D, V, R, W) &&
                             comic_beam_logits_pack_bytes(D, V) <= (int64_t)(D + 1) * wo_pad_cols(V) * 4 &&
                             comic_beam_logits_partial_floats(D, V, R, W, max_steps) <= (int64_t)R * V;
  // small vocabularies (radix-256): the entry's beam step with a beam's logits in a wave's registers; with the step's y at
  // hand as fragments (streaming LSTM step) the projection goes through the streaming kernel too
  const bool small_step = fused && lpw == 0.f && !stream_logits && beam_logits_enabled() && comic_beam_step_small_supported(V, W) &&
                          max_steps <= kBeamCntSteps;
  const bool stream_wo = small_step && stream_lstm && comic_stream_gemm_supported(D, V, R) &&
                         comic_stream_gemm_part_bytes(D, V, R) <= kSplitKBytes &&
                         comic_stream_gemm_wfrag_floats(D, V) <= (int64_t)(D + 1) * wo_pad_cols(V);
  if (stream_logits) {
    RC(comic_beam_pack_wo(p->W_o, p->b_o, V, ws.wo_pad, D, V, st));
    RC(comic_beam_logits_begin(ws.logits, B, W, V, max_steps, st));
  } else if (stream_wo) {
    RC(comic_stream_gemm_pack(p->W_o, ws.wo_pad, D, V, st));
    // (not with the context layer: its product after the attention may use the whole split-K scratch)
    if (sm.wqfrag && !d->context_layer && comic_stream_gemm_part_bytes(D, D, R) <= kSplitKBytes / 2 &&
        comic_stream_gemm_part_bytes(D, V, R) <= kSplitKBytes / 2) {
      sm.wofrag = ws.wo_pad;       // one launch for the query and the vocabulary projection
      sm.wo_N = V;
    }
  } else {
    mem.w_o = aligned_w_o(d, p, ws.wo_pad, &mem.ld_wo, st);
  }
  if (small_step) RC(comic_beam_counters_zero(ws.beam_cnt, max_steps, st));
  g_beam_path = (stream_logits ? 1 : 0) | (stream_lstm ? 2 : 0) | (small_step ? 4 : 0);
  int cur = 0;
  struct StopScope {          // whatever way this call returns, no later launch sees the flag
    ~StopScope() { g_comic_stop = ComicStop(); }
  } stop_scope;
  for (int t = 0; t < max_steps; ++t) {
    // the launches of step t return at once when the loop ended at an earlier step (see common.h, ComicStop);
    // fused path only: every kernel of its step honours the flag (the unfused path's gathers index through
    // the parents of the step before, which a skipped step leaves unwritten)
    if (fused) {
      g_comic_stop.p = steps_executed;
      g_comic_stop.t = t;
    }
    int32_t* word = step_ids + (size_t)t * R;
    int32_t* parent = parent_ids + (size_t)t * R;
    const int nxt = cur ^ 1;
    float* att_new;
    StepBufs sb = beam_step_bufs(d, ws, fused, nxt, R, &att_new);
    if (fused) {
      // (with the streaming LSTM step the merge / the small step also gathers the next step's operand rows: raw c / h /
      // attention outputs of this step through the parents it has just chosen)
      const LstmPrepArgs prep{p->emb, att_new, sb.h2, sb.c2, (uint4*)ws.xfrag, ws.gtmp, E, A, D, V, (E + A + D + 31) / 32};
      const int32_t* ids_in = t == 0 ? ws.ids : step_ids + (size_t)(t - 1) * R;
      const int32_t* par_in = t == 0 ? nullptr : parent_ids + (size_t)(t - 1) * R;
      sm.skip_prep = (stream_lstm && (stream_logits || small_step) && t > 0) ? 1 : 0;
      sm.wo_part = nullptr;
      StreamBufs* smp = stream_lstm ? &sm : nullptr;
      RC(infer_step_lstm(d, p, ws.kpanel, ids_in, par_in, W, ws.c[cur], ws.h[cur], ws.att[cur], sb, ws.gtmp, R, st, smp));
      // (the two chains that hang off y -- query projection + attention, vocabulary projection + top-k -- measured
      // slower on two lanes than back to back: 98.5 vs 94.8 us per step, the fork / join of a 20 us branch costs more
      // than the overlap returns)
      if (stream_logits && stream_lstm && sm.wqfrag) {
        // projection launch first, with the query projection's workgroups riding on the CUs its chunks leave idle; the
        // attention step (which needs q) and the merge (which gathers the attention output) follow
        int n_q = 0, q_lds = 0;
        const LstmStreamArgs qa = comic_stream_gemm_args(ws.yfrag, ws.wqfrag, (float*)g_splitk_ws, R, D, D, &sm.q_S, &n_q, &q_lds,
                                                         std::max(8, 256 - comic_beam_logits_chunks(V)));
        RC(comic_beam_logits_launch(sb.y, ws.yfrag, ws.wo_pad, ws.logits, max_steps, B, W, D, V, &qa, n_q, q_lds, st));
        RC(infer_step_attend(d, p, mem.ad, ws.keys, mem.values, sb, attn_hist + (size_t)t * R * H * M, R, st, smp, mem.mem_div));
        RC(comic_beam_merge_launch(ws.logits, ws.log_probs, finished, lengths, word, parent, scores + (size_t)t * R,
                                   steps_executed, t, max_steps, B, W, V, d->end_id, &prep, st));
        cur = nxt;
        continue;
      }
      RC(infer_step_attend(d, p, mem.ad, ws.keys, mem.values, sb, attn_hist + (size_t)t * R * H * M, R, st, smp, mem.mem_div));
      if (stream_logits) {
        RC(comic_beam_logits_step(sb.y, stream_lstm ? ws.yfrag : nullptr, ws.wo_pad, ws.logits, ws.log_probs, finished, lengths, word, parent,
                                  scores + (size_t)t * R, steps_executed, t, max_steps, B, W, D, V, d->end_id,
                                  stream_lstm ? &prep : nullptr, st));
      } else if (small_step) {
        // small vocabulary: the entry's whole step in one workgroup, which also keeps steps_executed
        if (stream_wo) {     // vocabulary projection through the streaming kernel: K-slice partials, summed by the step kernel
          int S = sm.wo_S;
          const int ldp = (V + 63) / 64 * 64;
          const float* lp_part = sm.wo_part;               // launched together with the query projection ...
          if (!lp_part) {                                  // ... or on its own
            RC(comic_stream_gemm(ws.yfrag, ws.wo_pad, (float*)g_splitk_ws, kSplitKBytes, R, D, V, &S, st));
            lp_part = (const float*)g_splitk_ws;
          }
          RC(comic_beam_step_small(lp_part, p->b_o, S, ldp, (long)R * ldp, ws.log_probs, finished, lengths,
                                   word, parent, scores + (size_t)t * R, B, W, V, d->end_id, ws.beam_cnt + t, steps_executed,
                                   t, max_steps, &prep, st));
        } else {
          RC(gemm_big(sb.y, mem.w_o, ws.logits, p->b_o, R, V, D, D, mem.ld_wo, V, 0, 0, 0.f, st));
          RC(comic_beam_step_small(ws.logits, nullptr, 1, V, 0, ws.log_probs, finished, lengths, word, parent,
                                   scores + (size_t)t * R, B, W, V, d->end_id, ws.beam_cnt + t, steps_executed, t, max_steps,
                                   stream_lstm ? &prep : nullptr, st));
        }
      } else {
        RC(gemm_big(sb.y, mem.w_o, ws.logits, p->b_o, R, V, D, D, mem.ld_wo, V, 0, 0, 0.f, st));
        RC(comic_beam_step_ws(ws.logits, ws.log_probs, finished, lengths, word, parent, scores + (size_t)t * R, B, W, V,
                              d->end_id, lpw, g_splitk_ws, kSplitKBytes, st));
      }
    } else {
      if (t > 0) (void)hipMemcpyAsync(ws.ids, step_ids + (size_t)(t - 1) * R, sizeof(int32_t) * R,
                                      hipMemcpyDeviceToDevice, st);
      RC(comic_embed_fwd(p->emb, ws.ids, ws.x, R, E, V, (void*)st));
      RC(infer_step(d, p, mem.ad, ws.keys, mem.values, ws.x, ws.c[cur], ws.h[cur], ws.att[cur], sb,
                    attn_hist + (size_t)t * R * H * M, R, st));
      RC(gemm_big(sb.y, mem.w_o, ws.logits, p->b_o, R, V, D, D, mem.ld_wo, V, 0, 0, 0.f, st));
      RC(comic_beam_step_ws(ws.logits, ws.log_probs, finished, lengths, word, parent, scores + (size_t)t * R, B, W, V,
                            d->end_id, lpw, g_splitk_ws, kSplitKBytes, st));
      RC(comic_gather_rows(sb.c2, parent, ws.c[nxt], R, W, D, (void*)st));
      RC(comic_gather_rows(sb.h2, parent, ws.h[nxt], R, W, D, (void*)st));
      RC(comic_gather_rows(att_new, parent, ws.att[nxt], R, W, A, (void*)st));
    }
    if (!stream_logits && !small_step) {       // (the streaming step's merge / the small step keep steps_executed themselves)
      hipLaunchKernelGGL(all_finished_kernel, dim3(1), dim3(256), 0, st, finished, steps_executed, t, R, max_steps);
      COMIC_LAUNCH_CHECK("all_finished");
    }
    cur = nxt;
  }
  return 0;
}

// ---- ensemble beam search: several members, one beam ------------------------------------------------------------------------
// rnn_decoder_beam_search (ops_rnn.py:49-112) over the MEAN of the members' step distributions.  An executor of its own
// beside comic_decoder_beam: that loop picks one of three fused projection + top-k launches per shape, each of which owns a
// single member's W_o; here every member runs its own wrapper step on its own InferBufs, writes its logits into one slab,
// and one ensemble step (beam_step.hip) ranks the candidates for all of them.  Members follow the SAME ids / parents.
namespace {
// Workspace of the ensemble loop: the members' InferBufs one after another, then the shared blocks.  carve_ens is the ONE
// definition: comic_decoder_beam_search_workspace runs it over a null base.  A constrained loop (ban_steps > 0) adds the
// ban masks and the two history buffers of beam_bans.hip.
struct EnsBufs {
  InferBufs m[kEnsMax];
  float* alpha[kEnsMax];       // one step's [R][H][M] alignments of a member whose history nobody asked for
  float *logits, *log_probs;       // [n][R][V] slab, [R]
  int32_t* ids;                    // [R] start ids
  void* step_ws;
  int64_t step_bytes;
  uint32_t* bits;                  // [R][ceil(V / 32)] ban masks (constrained, truncated or prefixed only)
  int32_t* ban_hist;               // [2][R][max_steps] token histories in beam order (constrained only)
  void* trunc_ws;                  // comic_beam_truncate's scratch rows (truncated only; none while a row fits in LDS)
  int64_t trunc_bytes;
  int32_t *req_base, *req_special; // [R], [R][4][2]: the per-step table of beam_required.hip (required words only)
  size_t bytes;
  bool ok;
};
// bytes of the ensemble step's workspace for any split of `rows` into batch x beam: (2 n + 2) * rows * chunks words, chunks <= 32
int64_t ens_step_ws_bound(int n, int rows) { return comic_beam_step_split_bytes(n, rows, 1, 32); }
// sampled: the step's lists carry every slot's total too (comic_beam_step_sampled_workspace): rows * chunks words more
// truncated: the masks even without constraints, and the truncation's scratch rows
// required words (req_steps > 0): the banked step's state copy, the per-step table, and the histories unless the
// constraints keep them already
// prefixed: the masks even without constraints or truncation (the last block, so every other decode's layout stands)
struct EnsShape {
  int ban_steps;
  bool sampled, truncated;
  int req_steps;
  bool prefixed;
};
// The ONE derivation of that shape from "which options are present": the workspace query and the run both use it.
EnsShape ens_shape(const comic_beam_options& o, int max_steps, const comic_beam_prefix* prefix) {
  return EnsShape{o.constraints ? max_steps : 0, o.sampling != nullptr, o.truncation != nullptr, o.required ? max_steps : 0,
                  prefix != nullptr};
}
EnsBufs carve_ens(const comic_decoder_desc* descs, int n, int R, void* ws, int64_t bytes, const EnsShape& shape) {
  const int ban_steps = shape.ban_steps, req_steps = shape.req_steps;
  const bool sampled = shape.sampled, truncated = shape.truncated;
  EnsBufs e{};
  size_t off = 0;
  e.ok = true;
  for (int m = 0; m < n; ++m) {
    const int64_t left = std::max<int64_t>(0, bytes - (int64_t)off);
    e.m[m] = carve_infer(&descs[m], R, ws ? (char*)ws + off : nullptr, left, 0);
    e.ok = e.ok && e.m[m].ok;
    off += e.m[m].bytes;
  }
  Bump w(ws ? (char*)ws + off : nullptr, (size_t)std::max<int64_t>(0, bytes - (int64_t)off));
  for (int m = 0; m < n; ++m) e.alpha[m] = w.take<float>((size_t)R * descs[m].H * descs[m].M);
  e.logits = w.take<float>((size_t)n * R * descs[0].V);
  e.log_probs = w.take<float>(R);
  e.ids = w.take<int32_t>(R);
  e.step_bytes = ens_step_ws_bound(n, R) + (sampled ? (int64_t)R * 32 * 4 : 0);
  if (req_steps > 0) e.step_bytes = comic_beam_step_required_bytes(n, R, 1, 32);
  e.step_ws = w.take<char>((size_t)e.step_bytes);
  if (ban_steps > 0) {
    e.bits = w.take<uint32_t>((size_t)R * ((descs[0].V + 31) / 32));
    e.ban_hist = w.take<int32_t>((size_t)2 * R * ban_steps);
  }
  if (truncated) {
    if (ban_steps <= 0) e.bits = w.take<uint32_t>((size_t)R * ((descs[0].V + 31) / 32));
    e.trunc_bytes = std::max<int64_t>(0, comic_beam_truncate_workspace(n, R, 1, descs[0].V));
    if (e.trunc_bytes > 0) e.trunc_ws = w.take<char>((size_t)e.trunc_bytes);
  }
  if (req_steps > 0) {
    e.req_base = w.take<int32_t>(R);
    e.req_special = w.take<int32_t>((size_t)R * 8);
    if (ban_steps <= 0) e.ban_hist = w.take<int32_t>((size_t)2 * R * req_steps);
  }
  if (shape.prefixed && ban_steps <= 0 && !truncated) e.bits = w.take<uint32_t>((size_t)R * ((descs[0].V + 31) / 32));
  e.ok = e.ok && w.ok;
  e.bytes = off + w.off;
  return e;
}
}  // namespace

extern "C" int64_t comic_decoder_beam_search_prefixed_workspace(const comic_decoder_desc* descs, int n_models, int rows,
                                                                int max_steps, const comic_beam_options* options,
                                                                const comic_beam_prefix* prefix) {
  const comic_beam_options o = options ? *options : comic_beam_options{};
  if (!descs || n_models < 1 || n_models > kEnsMax || rows <= 0) return -1;
  for (int m = 0; m < n_models; ++m)
    if (descs[m].D <= 0 || descs[m].V <= 0 || descs[m].M <= 0 || descs[m].H <= 0) return -1;
  if ((o.constraints || o.required) && max_steps <= 0) return -1;
  if (o.truncation && comic_beam_truncate_workspace(n_models, rows, 1, descs[0].V) < 0) return -1;
  if (prefix && (prefix->max_tokens < 1 || prefix->max_tokens >= max_steps || descs[0].V > 65536)) return -1;
  return (int64_t)carve_ens(descs, n_models, rows, nullptr, 0, ens_shape(o, max_steps, prefix)).bytes;
}
extern "C" int64_t comic_decoder_beam_search_workspace(const comic_decoder_desc* descs, int n_models, int rows,
                                                       int max_steps, const comic_beam_options* options) {
  return comic_decoder_beam_search_prefixed_workspace(descs, n_models, rows, max_steps, options, nullptr);
}

// The ONE ensemble loop.  cons null: comic_decoder_beam_ensemble, launch for launch as it always was; else every step
// builds the beams' ban masks first (beam_bans.hip) and ranks through them (the Bans policy of beam_step.hip).  grp null:
// one beam of width W; else the first slot of every group starts live and every step ranks under the Groups policy.  smp
// null: no sampling; else (grp is one group at the most) every slot starts live and step t ranks under the Samples policy.
// trc null: no truncation; else (smp is not null) every step narrows the mask by top-k / top-p (beam_truncate.hip) before
// it ranks.  rqd null: no required words; else (no sampling, one group at the most, which is no groups) the banks.
// prefix null: no forced prefix; else the first P = max_tokens steps write the forcing masks (beam_prefix.hip) over the
// constraints' and rank through L.bits whichever policy is on; from step P on the launches are those of a null prefix.
extern "C" int comic_decoder_beam_search_prefixed(const comic_decoder_desc* descs, const comic_decoder_params* params,
                                                  const float* const* fms, const float* const* im_embeds,
                                                  const float* weights, int n_models, int B, int W, int max_steps,
                                                  const comic_beam_options* options, const comic_beam_prefix* prefix,
                                                  const int32_t* pfx, int32_t* step_ids, int32_t* parent_ids, float* scores,
                                                  int64_t* lengths, int32_t* finished, float* const* attn_hists,
                                                  int32_t* steps_executed, void* workspace, int64_t workspace_bytes,
                                                  void* stream) {
  const comic_beam_options o = options ? *options : comic_beam_options{};
  COMIC_REQUIRE(!prefix || pfx, "beam_prefixed: null prefix table");
  COMIC_REQUIRE(!prefix || (prefix->max_tokens >= 1 && prefix->max_tokens < max_steps),
                "beam_prefixed: max_tokens %d outside [1,%d)", prefix ? prefix->max_tokens : 0, max_steps);
  const int P = prefix ? prefix->max_tokens : 0;
  const comic_beam_constraints* cons = o.constraints;
  const comic_beam_sampling* smp = o.sampling;
  const comic_beam_truncation* trc = o.truncation;
  const comic_beam_required* rqd = o.required;
  const comic_beam_groups* grp = rqd ? nullptr : o.groups;
  const int32_t* req = o.req;
  COMIC_REQUIRE(!rqd || !o.groups || o.groups->groups <= 1, "beam_required: groups = %d does not combine with required words",
                o.groups ? o.groups->groups : 0);
  COMIC_REQUIRE(!rqd || !smp, "beam_required: sampling does not combine with required words");
  COMIC_REQUIRE(!smp || !grp || grp->groups <= 1, "beam_sampled: sampling does not combine with groups = %d",
                grp ? grp->groups : 0);
  COMIC_REQUIRE(!trc || smp, "beam_truncated: null sampling");
  COMIC_REQUIRE(!rqd || req, "beam_required: null req table");
  COMIC_REQUIRE(descs && params && fms && im_embeds && weights && step_ids && parent_ids && scores && lengths && finished &&
                    steps_executed && workspace,
                "beam_ensemble: null pointer");
  COMIC_REQUIRE(n_models >= 1 && n_models <= kEnsMax, "beam_ensemble: 1 to %d members (got %d)", kEnsMax, n_models);
  COMIC_REQUIRE(B > 0 && W > 0 && W <= 64 && max_steps > 0, "beam_ensemble: bad shape");
  const int n = n_models, R = B * W, V = descs[0].V;
  for (int m = 0; m < n; ++m) {
    RC(check_desc(&descs[m]));
    RC(check_cell_params(&descs[m], &params[m]));
    COMIC_REQUIRE(fms[m] && im_embeds[m], "beam_ensemble: member %d has no features", m);
    COMIC_REQUIRE(descs[m].V == V && descs[m].start_id == descs[0].start_id && descs[m].end_id == descs[0].end_id,
                  "beam_ensemble: member %d differs from member 0 in V / start_id / end_id", m);
  }
  COMIC_REQUIRE(W <= V && (long)W * V < (1L << 31), "beam_ensemble: beam*V too large or beam > V");
  if (cons) RC(comic_beam_constraints_check(cons, "beam_constrained", W, V, descs[0].end_id, max_steps, true));
  if (grp) RC(comic_beam_groups_check(grp, "beam_diverse", W, V));
  if (smp) RC(comic_beam_sampling_check(smp, trc ? "beam_truncated" : "beam_sampled", descs[0].length_penalty_weight, W));
  if (trc) RC(comic_beam_truncation_check(trc, "beam_truncated", V, true));
  if (rqd) RC(comic_beam_required_check(rqd, "beam_required", W, V, descs[0].end_id, max_steps, cons));
  if (prefix) RC(comic_beam_prefix_check(prefix, "beam_prefixed", V, max_steps));
  hipStream_t st = (hipStream_t)stream;
  EnsBufs L = carve_ens(descs, n, R, workspace, workspace_bytes, ens_shape(o, max_steps, prefix));
  COMIC_REQUIRE(L.ok && (int64_t)L.bytes <= workspace_bytes, "beam_ensemble: workspace too small");
  g_splitk_ws = L.m[0].splitk;               // members run back to back on the one stream: one split-K scratch serves all
  const float lpw = descs[0].length_penalty_weight;
  BeamMember mem[kEnsMax];
  for (int m = 0; m < n; ++m) {
    const comic_decoder_desc* d = &descs[m];
    const comic_decoder_params* p = &params[m];
    FlagScope flag_scope__(d);
    InferBufs& ws = L.m[m];
    BeamMember& e = mem[m];
    RC(beam_member_begin(d, p, fms[m], im_embeds[m], B, W, ws, st, e));
    e.w_o = aligned_w_o(d, p, ws.wo_pad, &e.ld_wo, st);
  }
  // (groups: row i starts live when i % Wg == 0, the first slot of its group; sampling: every row; required words: the
  // first slot of the bank that the entry's padding rows select)
  if (rqd)
    RC(comic_beam_required_init_launch(req, L.log_probs, finished, lengths, B, W, rqd, st));
  else
    hipLaunchKernelGGL(beam_init_kernel, dim3(cdiv(R, 256)), dim3(256), 0, st, L.log_probs, finished, lengths, R,
                       smp ? 1 : grp ? W / grp->groups : W);
  hipLaunchKernelGGL(fill_i32_kernel, dim3(cdiv(R, 256)), dim3(256), 0, st, L.ids, descs[0].start_id, (long)R);
  hipLaunchKernelGGL(fill_i32_kernel, dim3(1), dim3(64), 0, st, steps_executed, max_steps, 1L);
  COMIC_LAUNCH_CHECK("beam_ensemble init");
  struct StopScope {          // whatever way this call returns, no later launch sees the flag
    ~StopScope() { g_comic_stop = ComicStop(); }
  } stop_scope;
  for (int t = 0; t < max_steps; ++t) {
    // the launches of step t return at once when the loop ended at an earlier step (common.h, ComicStop).  Members on
    // the per-step launch chain keep running on their last state; what they index through (ids: clamped by the embedding
    // kernel, parents: comic_ens_gather_state) tolerates the unwritten rows of a skipped step.
    g_comic_stop.p = steps_executed;
    g_comic_stop.t = t;
    int32_t* word = step_ids + (size_t)t * R;
    int32_t* parent = parent_ids + (size_t)t * R;
    const int32_t* ids_in = t == 0 ? L.ids : step_ids + (size_t)(t - 1) * R;
    const int32_t* par_in = t == 0 ? nullptr : parent_ids + (size_t)(t - 1) * R;
    for (int m = 0; m < n; ++m) {
      const comic_decoder_desc* d = &descs[m];
      const comic_decoder_params* p = &params[m];
      FlagScope flag_scope__(d);
      InferBufs& ws = L.m[m];
      BeamMember& e = mem[m];
      const int D = d->D, E = d->E, A = d->A;
      float* hist = (attn_hists && attn_hists[m]) ? attn_hists[m] + (size_t)t * R * d->H * d->M : L.alpha[m];
      float* lg = L.logits + (size_t)m * R * V;
      const int cur = e.cur, nxt = cur ^ 1;
      float* att_new;
      StepBufs sb = beam_step_bufs(d, ws, e.fused, nxt, R, &att_new);
      if (e.fused) {
        e.sm.skip_prep = 0;
        e.sm.wo_part = nullptr;
        StreamBufs* smp = e.stream_lstm ? &e.sm : nullptr;
        RC(infer_step_lstm(d, p, ws.kpanel, ids_in, par_in, W, ws.c[cur], ws.h[cur], ws.att[cur], sb, ws.gtmp, R, st, smp));
        RC(infer_step_attend(d, p, e.ad, ws.keys, e.values, sb, hist, R, st, smp, e.mem_div));
        e.cur = nxt;
      } else {
        if (t > 0) RC(comic_ens_gather_state(sb.c2, sb.h2, att_new, par_in, ws.c[0], ws.h[0], ws.att[0], R, W, D, A, st));
        RC(comic_embed_fwd(p->emb, ids_in, ws.x, R, E, V, (void*)st));
        RC(infer_step(d, p, e.ad, ws.keys, e.values, ws.x, ws.c[0], ws.h[0], ws.att[0], sb, hist, R, st));
      }
      RC(gemm_big(sb.y, e.w_o, lg, p->b_o, R, V, D, D, e.ld_wo, V, 0, 0, 0.f, st));
    }
    if (cons)
      RC(comic_beam_bans_launch(t == 0 ? nullptr : (const int32_t*)ids_in, par_in, finished, lengths, L.ban_hist, L.bits, t, B,
                                W, V, max_steps, descs[0].end_id, cons, st));
    // (inside the prefix the forcing masks go over the constraints'; from here on `masked` is what `cons` was)
    const bool forcing = t < P;
    const bool masked = cons || forcing;
    if (forcing) RC(comic_beam_prefix_launch(pfx, finished, L.bits, t, B, W, V, P, cons ? 1 : 0, st));
    if (trc)
      RC(comic_beam_truncate(L.logits, weights, n, finished, L.bits, (V + 31) / 32, B, W, V, smp->temperature, trc,
                             masked ? 1 : 0, L.trunc_ws, L.trunc_bytes, (void*)st));
    if (rqd) {
      // (with constraints the ban launch above has advanced the ONE pair of histories; this launch only reads them)
      RC(comic_beam_required_launch(t == 0 ? nullptr : (const int32_t*)ids_in, par_in, req, L.ban_hist, L.req_base,
                                    L.req_special, rqd, t, B, W, V, max_steps, cons ? 0 : 1, st));
      RC(comic_beam_step_required(L.logits, weights, n, L.log_probs, finished, lengths, word, parent, scores + (size_t)t * R,
                                  B, W, V, descs[0].end_id, lpw, masked ? L.bits : nullptr, (V + 31) / 32, L.req_base,
                                  L.req_special, rqd->n_words * rqd->stride + 1, L.step_ws, L.step_bytes, (void*)st));
    } else if (smp) {
      RC(comic_beam_step_sampled(L.logits, weights, n, L.log_probs, finished, lengths, word, parent, scores + (size_t)t * R,
                                 B, W, V, descs[0].end_id, (masked || trc) ? L.bits : nullptr, (V + 31) / 32, smp, t, L.step_ws,
                                 L.step_bytes, (void*)st));
    } else if (grp) {
      RC(comic_beam_step_diverse(L.logits, weights, n, L.log_probs, finished, lengths, word, parent, scores + (size_t)t * R,
                                 B, W, V, descs[0].end_id, lpw, masked ? L.bits : nullptr, (V + 31) / 32, grp, L.step_ws,
                                 L.step_bytes, (void*)st));
    } else if (masked) {
      RC(comic_beam_step_constrained(L.logits, weights, n, L.log_probs, finished, lengths, word, parent,
                                     scores + (size_t)t * R, B, W, V, descs[0].end_id, lpw, L.bits, (V + 31) / 32, L.step_ws,
                                     L.step_bytes, (void*)st));
    } else {
      RC(comic_beam_step_ensemble(L.logits, weights, n, L.log_probs, finished, lengths, word, parent, scores + (size_t)t * R,
                                  B, W, V, descs[0].end_id, lpw, L.step_ws, L.step_bytes, (void*)st));
    }
    hipLaunchKernelGGL(all_finished_kernel, dim3(1), dim3(256), 0, st, finished, steps_executed, t, R, max_steps);
    COMIC_LAUNCH_CHECK("all_finished");
  }
  return 0;
}

extern "C" int comic_decoder_beam_search(const comic_decoder_desc* descs, const comic_decoder_params* params,
                                         const float* const* fms, const float* const* im_embeds, const float* weights,
                                         int n_models, int B, int W, int max_steps, const comic_beam_options* options,
                                         int32_t* step_ids, int32_t* parent_ids, float* scores, int64_t* lengths,
                                         int32_t* finished, float* const* attn_hists, int32_t* steps_executed,
                                         void* workspace, int64_t workspace_bytes, void* stream) {
  return comic_decoder_beam_search_prefixed(descs, params, fms, im_embeds, weights, n_models, B, W, max_steps, options,
                                            nullptr, nullptr, step_ids, parent_ids, scores, lengths, finished, attn_hists,
                                            steps_executed, workspace, workspace_bytes, stream);
}

// ---- the named per-option entries: the frozen version-1 forms -----------------------------------------------------------------
// Each is its own null checks and one forwarding call.  A workspace query knows its options by their presence alone.
namespace {
comic_beam_options present(int cons, bool smp = false, bool trc = false, bool rqd = false) {
  static const comic_beam_constraints c{};
  static const comic_beam_sampling s{};
  static const comic_beam_truncation t{};
  static const comic_beam_required r{};
  return comic_beam_options{cons ? &c : nullptr, nullptr, smp ? &s : nullptr, trc ? &t : nullptr, rqd ? &r : nullptr, nullptr};
}
}  // namespace

extern "C" int64_t comic_decoder_beam_ensemble_workspace(const comic_decoder_desc* descs, int n_models, int rows,
                                                         int max_steps) {
  return comic_decoder_beam_search_workspace(descs, n_models, rows, max_steps, nullptr);
}
extern "C" int64_t comic_decoder_beam_constrained_workspace(const comic_decoder_desc* descs, int n_models, int rows,
                                                            int max_steps) {
  const comic_beam_options o = present(1);
  return comic_decoder_beam_search_workspace(descs, n_models, rows, max_steps, &o);
}
extern "C" int64_t comic_decoder_beam_diverse_workspace(const comic_decoder_desc* descs, int n_models, int rows,
                                                        int max_steps, int constrained) {
  const comic_beam_options o = present(constrained);
  return comic_decoder_beam_search_workspace(descs, n_models, rows, max_steps, &o);
}
extern "C" int64_t comic_decoder_beam_sampled_workspace(const comic_decoder_desc* descs, int n_models, int rows,
                                                        int max_steps, int constrained) {
  const comic_beam_options o = present(constrained, true);
  return comic_decoder_beam_search_workspace(descs, n_models, rows, max_steps, &o);
}
extern "C" int64_t comic_decoder_beam_truncated_workspace(const comic_decoder_desc* descs, int n_models, int rows,
                                                          int max_steps, int constrained) {
  const comic_beam_options o = present(constrained, true, true);
  return comic_decoder_beam_search_workspace(descs, n_models, rows, max_steps, &o);
}
extern "C" int64_t comic_decoder_beam_required_workspace(const comic_decoder_desc* descs, int n_models, int rows,
                                                         int max_steps, int constrained) {
  const comic_beam_options o = present(constrained, false, false, true);
  return comic_decoder_beam_search_workspace(descs, n_models, rows, max_steps, &o);
}

extern "C" int comic_decoder_beam_ensemble(const comic_decoder_desc* descs, const comic_decoder_params* params,
                                           const float* const* fms, const float* const* im_embeds, const float* weights,
                                           int n_models, int B, int W, int max_steps, int32_t* step_ids, int32_t* parent_ids,
                                           float* scores, int64_t* lengths, int32_t* finished, float* const* attn_hists,
                                           int32_t* steps_executed, void* workspace, int64_t workspace_bytes, void* stream) {
  return comic_decoder_beam_search(descs, params, fms, im_embeds, weights, n_models, B, W, max_steps, nullptr, step_ids,
                                   parent_ids, scores, lengths, finished, attn_hists, steps_executed, workspace,
                                   workspace_bytes, stream);
}

extern "C" int comic_decoder_beam_constrained(const comic_decoder_desc* descs, const comic_decoder_params* params,
                                              const float* const* fms, const float* const* im_embeds, const float* weights,
                                              int n_models, int B, int W, int max_steps,
                                              const comic_beam_constraints* constraints, int32_t* step_ids,
                                              int32_t* parent_ids, float* scores, int64_t* lengths, int32_t* finished,
                                              float* const* attn_hists, int32_t* steps_executed, void* workspace,
                                              int64_t workspace_bytes, void* stream) {
  COMIC_REQUIRE(constraints, "beam_constrained: null constraints");
  const comic_beam_options o{constraints, nullptr, nullptr, nullptr, nullptr, nullptr};
  return comic_decoder_beam_search(descs, params, fms, im_embeds, weights, n_models, B, W, max_steps, &o, step_ids,
                                   parent_ids, scores, lengths, finished, attn_hists, steps_executed, workspace,
                                   workspace_bytes, stream);
}

extern "C" int comic_decoder_beam_diverse(const comic_decoder_desc* descs, const comic_decoder_params* params,
                                          const float* const* fms, const float* const* im_embeds, const float* weights,
                                          int n_models, int B, int W, int max_steps,
                                          const comic_beam_constraints* constraints, const comic_beam_groups* groups,
                                          int32_t* step_ids, int32_t* parent_ids, float* scores, int64_t* lengths,
                                          int32_t* finished, float* const* attn_hists, int32_t* steps_executed,
                                          void* workspace, int64_t workspace_bytes, void* stream) {
  COMIC_REQUIRE(groups, "beam_diverse: null groups");
  const comic_beam_options o{constraints, groups, nullptr, nullptr, nullptr, nullptr};
  return comic_decoder_beam_search(descs, params, fms, im_embeds, weights, n_models, B, W, max_steps, &o, step_ids,
                                   parent_ids, scores, lengths, finished, attn_hists, steps_executed, workspace,
                                   workspace_bytes, stream);
}

extern "C" int comic_decoder_beam_sampled(const comic_decoder_desc* descs, const comic_decoder_params* params,
                                          const float* const* fms, const float* const* im_embeds, const float* weights,
                                          int n_models, int B, int W, int max_steps,
                                          const comic_beam_constraints* constraints, const comic_beam_sampling* sampling,
                                          int32_t* step_ids, int32_t* parent_ids, float* scores, int64_t* lengths,
                                          int32_t* finished, float* const* attn_hists, int32_t* steps_executed,
                                          void* workspace, int64_t workspace_bytes, void* stream) {
  COMIC_REQUIRE(sampling, "beam_sampled: null sampling");
  const comic_beam_options o{constraints, nullptr, sampling, nullptr, nullptr, nullptr};
  return comic_decoder_beam_search(descs, params, fms, im_embeds, weights, n_models, B, W, max_steps, &o, step_ids,
                                   parent_ids, scores, lengths, finished, attn_hists, steps_executed, workspace,
                                   workspace_bytes, stream);
}

extern "C" int comic_decoder_beam_truncated(const comic_decoder_desc* descs, const comic_decoder_params* params,
                                            const float* const* fms, const float* const* im_embeds, const float* weights,
                                            int n_models, int B, int W, int max_steps,
                                            const comic_beam_constraints* constraints, const comic_beam_sampling* sampling,
                                            const comic_beam_truncation* truncation, int32_t* step_ids, int32_t* parent_ids,
                                            float* scores, int64_t* lengths, int32_t* finished, float* const* attn_hists,
                                            int32_t* steps_executed, void* workspace, int64_t workspace_bytes,
                                            void* stream) {
  COMIC_REQUIRE(sampling, "beam_truncated: null sampling");
  COMIC_REQUIRE(truncation, "beam_truncated: null truncation");
  const comic_beam_options o{constraints, nullptr, sampling, truncation, nullptr, nullptr};
  return comic_decoder_beam_search(descs, params, fms, im_embeds, weights, n_models, B, W, max_steps, &o, step_ids,
                                   parent_ids, scores, lengths, finished, attn_hists, steps_executed, workspace,
                                   workspace_bytes, stream);
}

extern "C" int comic_decoder_beam_required(const comic_decoder_desc* descs, const comic_decoder_params* params,
                                           const float* const* fms, const float* const* im_embeds, const float* weights,
                                           int n_models, int B, int W, int max_steps,
                                           const comic_beam_constraints* constraints, const comic_beam_groups* groups,
                                           const comic_beam_sampling* sampling, const comic_beam_required* required,
                                           const int32_t* req, int32_t* step_ids, int32_t* parent_ids, float* scores,
                                           int64_t* lengths, int32_t* finished, float* const* attn_hists,
                                           int32_t* steps_executed, void* workspace, int64_t workspace_bytes, void* stream) {
  COMIC_REQUIRE(required, "beam_required: null required");
  COMIC_REQUIRE(req, "beam_required: null req table");
  const comic_beam_options o{constraints, groups, sampling, nullptr, required, req};
  return comic_decoder_beam_search(descs, params, fms, im_embeds, weights, n_models, B, W, max_steps, &o, step_ids,
                                   parent_ids, scores, lengths, finished, attn_hists, steps_executed, workspace,
                                   workspace_bytes, stream);
}
