// Executor-only forms of the decoder step kernels (decoder.hip, cells.hip, gemm.hip): ONE list of prototypes for the
// two translation units that call them -- the executors (decoder_exec.hip) and the op-level C entries of the test
// suite (op_entries.hip).  The public ops of include/comic_hip.h reach these with every executor-only argument null,
// 0 or 1; training, greedy / beam decode, sampling and scoring launch the forms below.
#pragma once
#include "common.h"

// plain queries and the split-K product: exported under their own names (C linkage; declared in include/comic_hip.h)
extern "C" {
int comic_attn_splits(int B, int M);
long comic_attn_bwd_scratch(int B, int H, int M, int D);
int comic_cell_ln_stride(int D);
int comic_gemm_f32_partial(const float* A, const float* B, int M, int N, int K, int lda, int ldb, int trans_b, void* ws,
                           int64_t ws_bytes, int* S_out, void* stream);
}

// decoder.hip
int comic_xent_ex(float* logits, const int32_t* targets_bt, const float* coef_bt, const float* wmask_bt,
                  const int32_t* lens, float* loss_rows, float* dlogits, int32_t* ids_tb, int t_rows, int t_stride,
                  int B, int V, hipStream_t st);
int comic_xent_maploss(float* logits, const int32_t* targets_bt, const float* coef_bt, const float* wmask_bt,
                       const int32_t* lens, float* loss_rows, float* dlogits, int ld_dl, int32_t* ids_tb, int t_rows,
                       int t_stride, int B, int V, const float* hist, float* dmap, float* partial, float* map_loss,
                       unsigned* ticket, int H, int M, float scale, hipStream_t st);
int comic_attn_fwd_ex(const comic_attn_desc* d, const float* keys, const float* values, const float* q,
                      const float* ln_g, const float* ln_b, const float* v, const float* tau, const float* mask_alpha,
                      float keep_alpha, float* alpha, float* alpha_d, float* ctx, const int32_t* lens, int t,
                      const float* att_prev, float* att_next, float* xh_next, int xh_ld, const float* mask_next,
                      int mask_ld, float keep_in, int q_parts, float* q_out, float* scores_ws, hipStream_t st,
                      int mem_div = 1);
int comic_attn_bwd_ex(const comic_attn_desc* d, const float* keys, const float* values, const float* q,
                      const float* ln_g, const float* ln_b, const float* v, const float* tau, const float* alpha,
                      const float* mask_alpha, float keep_alpha, const float* dctx, const float* dmap, float* dq,
                      float* dkeys, float* dvalues, float* pgrad, const int32_t* lens, int t, hipStream_t st,
                      int pgrad_overwrite, float* ws_s = nullptr, float* ws_d = nullptr);
int comic_lstm_gates_fwd_ex(const float* g, const float* c_prev, const float* h_prev, float* gates_act, float* c_new,
                            float* y, const float* mask_out, float keep_out, const int32_t* lens, int t,
                            float* c_state, float* h_state, int B, int D, float* xh_next, int xh_ld, int S,
                            const float* bias, hipStream_t st);
int comic_lstm_gates_bwd_ex(const float* gates_act, const float* c_prev, const float* c_new, const float* dy,
                            const float* dy_part, int S, const float* mask_out, float keep_out, const int32_t* lens,
                            int t, float* dc_state, float* dh_state, float* dg, int B, int D, hipStream_t st);
int comic_colsum_ws(const float* in, float* out, int rows, int cols, float beta, float* ws, hipStream_t st);

// the reference's other recurrent cells (cells.hip)
int comic_ln_lstm_fwd(const float* g, int S, const float* ln, const float* c_prev, const float* h_prev, float* gates_act,
                      float* xhat, float* rstd, float* c_new, float* y, const float* mask_out, float keep_out,
                      const int32_t* lens, int t, float* c_state, float* h_state, int B, int D, float* xh_next, int xh_ld,
                      hipStream_t st);
int comic_ln_lstm_bwd(const float* gates_act, const float* xhat, const float* rstd, const float* ln, const float* c_prev,
                      const float* c_new, const float* dy, const float* dy_part, int S, const float* mask_out,
                      float keep_out, const int32_t* lens, int t, float* dc, float* dh, float* dg, float* pgrad, int B, int D,
                      hipStream_t st);
int comic_ln_lstm_scatter(const float* sums, float* cell_ln_grad, int D, float beta, hipStream_t st);
int comic_gru_gates_fwd(const float* g1, int S, const float* bias, const float* h_prev, const float* xh, int xh_ld, float* ru,
                        int ld_ru, float* xh2, int xh2_ld, int B, int D, int EA, hipStream_t st);
int comic_gru_out_fwd(const float* g2, int S, const float* bias, const float* ru, int ld_ru, const float* h_prev,
                      float* cand, int ld_cand, float* y, const float* mask_out, float keep_out, const int32_t* lens, int t,
                      float* h_state, float* xh_next, int xh_ld, int B, int D, hipStream_t st);
int comic_gru_bwd1(const float* dy, const float* dy_part, int S, const float* mask_out, float keep_out, const int32_t* lens,
                   int t, float* dh_state, const float* ru, int ld_ru, const float* cand, int ld_cand, const float* h_prev,
                   float* dpre, int ld_dpre, int B, int D, hipStream_t st);
int comic_gru_bwd2(float* dxh2, int ld, const float* ru, int ld_ru, const float* h_prev, float* dpre, int ld_dpre, int B,
                   int D, int EA, hipStream_t st);
