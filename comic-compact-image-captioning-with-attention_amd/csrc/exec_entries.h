// Executor-only forms of the decoder step kernels (decoder.hip, cells.hip, gemm.hip, decoder_fused.hip, lstm_stream.hip,
// beam_logits.hip): ONE list of prototypes for the
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
// xent_soft.hip: the sequence loss against soft targets (row stride ld_dl of d logits; a null table with
// teacher_weight 0 is label smoothing alone)
int comic_xent_soft_ex(float* logits, const int32_t* targets_bt, const float* coef_bt, const float* wmask_bt,
                       const int32_t* lens, float* loss_rows, float* nll_rows, float* dlogits, int ld_dl, int32_t* ids_tb,
                       int t_rows, int t_stride, int B, int V, float smoothing, float teacher_weight, int K,
                       const int32_t* ids_tbk, const float* probs_tbk, hipStream_t st);
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

// the fused and streaming step kernels and the operand hand-off behind the beam merge (decoder_fused.hip,
// lstm_stream.hip, beam_logits.hip); the argument records: lstm_prep.h, lstm_stream_dev.h
struct LstmPrepArgs;
struct LstmStreamArgs;
// decoder_fused.hip
int comic_fused_step_supported(int D, int Wd);
long comic_lstm_panel_floats(int D, int Wd, int mode);
int comic_pack_lstm_panels(const float* K, float* fwd_panel, float* bwd_panel, int D, int Wd, hipStream_t st);
int comic_lstm_step_fused(const float* xh, int ld_xh, const float* K, const float* bias, const float* c_prev,
                          const float* h_prev, float* gates_act, float* c_new, float* y, const float* mask_out,
                          float keep_out, const int32_t* lens, int t, float* c_state, float* h_state, float* xh_next,
                          int xh_ld, int B, int D, int Wd, hipStream_t st);
int comic_pack_wq_panel(const float* Wq, float* panel, int D, hipStream_t st);
int comic_lstm_grad_fused(const float* dq, const float* wq_panel, const float* gates_act, const float* c_prev,
                          const float* c_new, const float* dy, const float* mask_out, float keep_out,
                          const int32_t* lens, int t, float* dc_state, float* dh_state, float* dg, int B, int D,
                          hipStream_t st);
int comic_input_grad_fused(const float* dg, const float* K, const float* mask, float keep, float* demb, float* datt,
                           float* dh, const int32_t* lens, int t, int carry, int B, int E, int A, int D,
                           hipStream_t st);
// lstm_stream.hip, beam_logits.hip
bool comic_lstm_stream_supported(int D, int E, int A, int R);
int64_t comic_lstm_stream_kfrag_floats(int D, int Wd);
int64_t comic_lstm_stream_xfrag_floats(int R, int Wd);
int64_t comic_lstm_stream_part_bytes(int D, int Wd, int R);
int comic_lstm_stream_pack(const float* K, void* k_frag, int D, int Wd, hipStream_t st);
int comic_lstm_stream_step(const float* table, const int32_t* ids, const int32_t* parent, int W, const float* att_src,
                           const float* h_src, const float* c_src, const void* k_frag, const float* bias, void* x_frag,
                           float* c_in, float* part, int64_t part_bytes, float* c_state, float* h_state, float* y,
                           void* y_frag, int R, int E, int A, int D, int V, int skip_prep, hipStream_t st);
bool comic_stream_gemm_supported(int Kin, int N, int R);
int64_t comic_stream_gemm_wfrag_floats(int Kin, int N);
int64_t comic_stream_gemm_part_bytes(int Kin, int N, int R);
int comic_stream_gemm_pack(const float* Wm, void* w_frag, int Kin, int N, hipStream_t st);
int comic_stream_gemm(const void* x_frag, const void* w_frag, float* part, int64_t part_bytes, int R, int Kin, int N, int* S,
                      hipStream_t st);
LstmStreamArgs comic_stream_gemm_args(const void* x_frag, const void* w_frag, float* part, int R, int Kin, int N, int* S,
                                      int* n_wg, int* lds_bytes, int max_wg);
int comic_beam_logits_chunks(int V);
int comic_beam_logits_launch(const float* y, const void* y_frag_in, const void* wo_frag, float* partials, int max_steps, int B,
                             int W, int D, int V, const LstmStreamArgs* q, int n_q, int q_lds, hipStream_t st);
int comic_beam_merge_launch(float* partials, float* log_probs, int32_t* finished, int64_t* lengths, int32_t* word_ids,
                            int32_t* parent_ids, float* scores, int32_t* steps_executed, int t, int max_steps, int B, int W,
                            int V, int end_id, const LstmPrepArgs* prep, hipStream_t st);
int comic_stream_gemm2(const void* x_frag, const void* w_a, float* part_a, int N_a, int* S_a, const void* w_b, float* part_b,
                       int N_b, int* S_b, int64_t part_bytes_each, int R, int Kin, hipStream_t st);
bool comic_beam_step_small_supported(int V, int W);
int comic_beam_counters_zero(void* cnt, int n, hipStream_t st);
int comic_beam_step_small(const float* logits, const float* bias, int S, int ld, long slice_stride, float* log_probs,
                          int32_t* finished, int64_t* lengths, int32_t* word_ids, int32_t* parent_ids, float* scores, int B,
                          int W, int V, int end_id, void* cnt, int32_t* steps_executed, int t, int max_steps,
                          const LstmPrepArgs* prep, hipStream_t st);
// beam_logits.hip
bool comic_beam_logits_supported(int D, int V, int R, int W);
int64_t comic_beam_logits_pack_bytes(int D, int V);
int64_t comic_beam_logits_partial_floats(int D, int V, int R, int W, int max_steps);
int comic_beam_logits_begin(float* partials, int B, int W, int V, int max_steps, hipStream_t st);
int comic_beam_pack_wo(const float* W_o, const float* b_o, int ld, void* wo_frag, int D, int V, hipStream_t st);
int comic_beam_logits_step(const float* y, const void* y_frag_in, const void* wo_frag, float* partials, float* log_probs,
                           int32_t* finished, int64_t* lengths, int32_t* word_ids, int32_t* parent_ids, float* scores,
                           int32_t* steps_executed, int t, int max_steps, int B, int W, int D, int V, int end_id,
                           const LstmPrepArgs* prep, hipStream_t st);
