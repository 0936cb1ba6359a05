// Decoding kernels around the beam step (beam_step.hip): row argmax (greedy), parent gathers, gather_tree.
//
// Restates tf.contrib.seq2seq [TF-1.9] as used by common/ops_rnn.py:49-180:
//   GreedyEmbeddingHelper.sample = argmax (lowest index wins ties)
//   gather_tree: back-track parents from max_len-1, EOS-fill after the first EOS.
#include "beam_select.h"

namespace {

// noise (may be null): per-element Gumbel noise of SampleEmbeddingHelper's categorical draw -- argmax(logits + g) is a
// sample of softmax(logits)
__global__ __launch_bounds__(256) void argmax_rows_kernel(const float* __restrict__ x, const float* __restrict__ noise,
                                                          int32_t* __restrict__ idx, int V) {
  __shared__ ValIdx sh[256];
  const float* row = x + (size_t)blockIdx.x * V;
  const float* nrow = noise ? noise + (size_t)blockIdx.x * V : nullptr;
  float bv = -INFINITY;
  int bi = kNone;
  for (int v = threadIdx.x; v < V; v += 256) {
    const float t = nrow ? row[v] + nrow[v] : row[v];
    if (better(t, v, bv, bi)) {
      bv = t;
      bi = v;
    }
  }
  const ValIdx r = block_argmax(bv, bi, sh);
  if (threadIdx.x == 0) idx[blockIdx.x] = r.i == kNone ? 0 : r.i;
}

__global__ void gather_rows_kernel(const float* __restrict__ in, const int32_t* __restrict__ parent,
                                   float* __restrict__ out, long total, int W, int cols) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int r = (int)(i / cols), c = (int)(i % cols);
  const int src = (r / W) * W + parent[r];
  out[i] = in[(size_t)src * cols + c];
}

// State re-ordering of a member that runs the per-step launch chain: out[r] = in[(r / W) * W + parent[r]] for c, h and the
// attention state in one launch.  Unlike gather_rows it honours the loop's stop flag and clamps the parent: after the loop
// has ended the previous step's parents were never written.
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

__global__ void gather_tree_kernel(const int32_t* __restrict__ step_ids, const int32_t* __restrict__ parent_ids,
                                   const int32_t* __restrict__ max_len, int32_t* __restrict__ out, int T, int B, int W,
                                   int end_id) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * W) return;
  const int b = i / W, w = i % W;
  for (int t = 0; t < T; ++t) out[((size_t)t * B + b) * W + w] = end_id;
  const int L = min(T, max_len[b]);
  if (L <= 0) return;
  out[((size_t)(L - 1) * B + b) * W + w] = step_ids[((size_t)(L - 1) * B + b) * W + w];
  int parent = parent_ids[((size_t)(L - 1) * B + b) * W + w];
  for (int level = L - 2; level >= 0; --level) {
    if (parent < 0 || parent >= W) return;  // invalid trajectory: leave EOS (reference raises)
    out[((size_t)level * B + b) * W + w] = step_ids[((size_t)level * B + b) * W + parent];
    parent = parent_ids[((size_t)level * B + b) * W + parent];
  }
  bool fin = false;
  for (int t = 0; t < L; ++t) {
    int32_t* p = out + ((size_t)t * B + b) * W + w;
    if (fin)
      *p = end_id;
    else if (*p == end_id)
      fin = true;
  }
}

}  // namespace

// executor-internal: argmax of x + noise (noise null: of x)
int comic_argmax_rows_noise(const float* x, const float* noise, int32_t* idx, int rows, int V, hipStream_t st) {
  COMIC_REQUIRE(x && idx && rows > 0 && V > 0, "argmax_rows: bad arguments");
  hipLaunchKernelGGL(argmax_rows_kernel, dim3(rows), dim3(256), 0, st, x, noise, idx, V);
  COMIC_LAUNCH_CHECK("argmax_rows");
  return 0;
}
extern "C" int comic_argmax_rows(const float* x, int32_t* idx, int rows, int V, void* stream) {
  return comic_argmax_rows_noise(x, nullptr, idx, rows, V, (hipStream_t)stream);
}

extern "C" int comic_gather_rows(const float* in, const int32_t* parent, float* out, int rows, int W, int cols,
                                 void* stream) {
  COMIC_REQUIRE(in != out, "gather_rows: in-place gather is not supported");
  const long total = (long)rows * cols;
  if (total == 0) return 0;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream, in,
                     parent, out, total, W, cols);
  COMIC_LAUNCH_CHECK("gather_rows");
  return 0;
}

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

extern "C" int comic_gather_tree(const int32_t* step_ids, const int32_t* parent_ids, const int32_t* max_len,
                                 int32_t* out, int T, int B, int W, int end_id, void* stream) {
  hipLaunchKernelGGL(gather_tree_kernel, dim3(cdiv(B * W, 64)), dim3(64), 0, (hipStream_t)stream, step_ids,
                     parent_ids, max_len, out, T, B, W, end_id);
  COMIC_LAUNCH_CHECK("gather_tree");
  return 0;
}
