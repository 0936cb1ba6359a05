// Op-level C entries of the executor-only kernel forms (include/comic_hip.h, "op-level entries of the executor-only
// forms"): each forwards its arguments to the internal entry of exec_entries.h and does nothing else, so a test can put
// one form on its own operands.  No product code calls these.
#include "exec_entries.h"

extern "C" {

int comic_op_attn_fwd(const comic_attn_desc* d, const float* keys, const float* values, const float* q, const float* ln_g,
                      const float* ln_b, const float* v, const float* tau, const float* mask_alpha, float keep_alpha,
                      float* alpha, float* alpha_d, float* ctx, const int32_t* lens, int t, const float* att_prev,
                      float* att_next, float* xh_next, int xh_ld, const float* mask_next, int mask_ld, float keep_in,
                      int q_parts, float* q_out, float* scores_ws, int mem_div, void* stream) {
  return comic_attn_fwd_ex(d, keys, values, q, ln_g, ln_b, v, tau, mask_alpha, keep_alpha, alpha, alpha_d, ctx, lens, t,
                           att_prev, att_next, xh_next, xh_ld, mask_next, mask_ld, keep_in, q_parts, q_out, scores_ws,
                           (hipStream_t)stream, mem_div);
}

int comic_op_attn_bwd(const comic_attn_desc* d, const float* keys, const float* values, const float* q, const float* ln_g,
                      const float* ln_b, const float* v, const float* tau, const float* alpha, const float* mask_alpha,
                      float keep_alpha, const float* dctx, const float* dmap, float* dq, float* dkeys, float* dvalues,
                      float* pgrad, const int32_t* lens, int t, int pgrad_overwrite, float* ws_s, float* ws_d,
                      void* stream) {
  return comic_attn_bwd_ex(d, keys, values, q, ln_g, ln_b, v, tau, alpha, mask_alpha, keep_alpha, dctx, dmap, dq, dkeys,
                           dvalues, pgrad, lens, t, (hipStream_t)stream, pgrad_overwrite, ws_s, ws_d);
}

int comic_op_xent(float* logits, const int32_t* targets_bt, const float* coef_bt, const float* wmask_bt,
                  const int32_t* lens, float* loss_rows, float* dlogits, int32_t* ids_tb, int t_rows, int t_stride, int B,
                  int V, void* stream) {
  return comic_xent_ex(logits, targets_bt, coef_bt, wmask_bt, lens, loss_rows, dlogits, ids_tb, t_rows, t_stride, B, V,
                       (hipStream_t)stream);
}

int comic_op_xent_maploss(float* logits, const int32_t* targets_bt, const float* coef_bt, const float* wmask_bt,
                          const int32_t* lens, float* loss_rows, float* dlogits, int ld_dl, int32_t* ids_tb, int t_rows,
                          int t_stride, int B, int V, const float* hist, float* dmap, float* partial, float* map_loss,
                          uint32_t* ticket, int H, int M, float scale, void* stream) {
  return comic_xent_maploss(logits, targets_bt, coef_bt, wmask_bt, lens, loss_rows, dlogits, ld_dl, ids_tb, t_rows,
                            t_stride, B, V, hist, dmap, partial, map_loss, ticket, H, M, scale, (hipStream_t)stream);
}

int comic_op_lstm_gates_fwd(const float* g, const float* c_prev, const float* h_prev, float* gates_act, float* c_new,
                            float* y, const float* mask_out, float keep_out, const int32_t* lens, int t, float* c_state,
                            float* h_state, int B, int D, float* xh_next, int xh_ld, int S, const float* bias,
                            void* stream) {
  return comic_lstm_gates_fwd_ex(g, c_prev, h_prev, gates_act, c_new, y, mask_out, keep_out, lens, t, c_state, h_state, B,
                                 D, xh_next, xh_ld, S, bias, (hipStream_t)stream);
}

int comic_op_lstm_gates_bwd(const float* gates_act, const float* c_prev, const float* c_new, const float* dy,
                            const float* dy_part, int S, const float* mask_out, float keep_out, const int32_t* lens, int t,
                            float* dc_state, float* dh_state, float* dg, int B, int D, void* stream) {
  return comic_lstm_gates_bwd_ex(gates_act, c_prev, c_new, dy, dy_part, S, mask_out, keep_out, lens, t, dc_state,
                                 dh_state, dg, B, D, (hipStream_t)stream);
}

int comic_op_colsum_ws(const float* in, float* out, int rows, int cols, float beta, float* ws, void* stream) {
  return comic_colsum_ws(in, out, rows, cols, beta, ws, (hipStream_t)stream);
}

int comic_op_ln_lstm_fwd(const float* g, int S, const float* ln, const float* c_prev, const float* h_prev,
                         float* gates_act, float* xhat, float* rstd, float* c_new, float* y, const float* mask_out,
                         float keep_out, const int32_t* lens, int t, float* c_state, float* h_state, int B, int D,
                         float* xh_next, int xh_ld, void* stream) {
  return comic_ln_lstm_fwd(g, S, ln, c_prev, h_prev, gates_act, xhat, rstd, c_new, y, mask_out, keep_out, lens, t, c_state,
                           h_state, B, D, xh_next, xh_ld, (hipStream_t)stream);
}

int comic_op_ln_lstm_bwd(const float* gates_act, const float* xhat, const float* rstd, const float* ln,
                         const float* c_prev, const float* c_new, const float* dy, const float* dy_part, int S,
                         const float* mask_out, float keep_out, const int32_t* lens, int t, float* dc, float* dh, float* dg,
                         float* pgrad, int B, int D, void* stream) {
  return comic_ln_lstm_bwd(gates_act, xhat, rstd, ln, c_prev, c_new, dy, dy_part, S, mask_out, keep_out, lens, t, dc, dh,
                           dg, pgrad, B, D, (hipStream_t)stream);
}

int comic_op_ln_lstm_scatter(const float* sums, float* cell_ln_grad, int D, float beta, void* stream) {
  return comic_ln_lstm_scatter(sums, cell_ln_grad, D, beta, (hipStream_t)stream);
}

int comic_op_gru_gates_fwd(const float* g1, int S, const float* bias, const float* h_prev, const float* xh, int xh_ld,
                           float* ru, int ld_ru, float* xh2, int xh2_ld, int B, int D, int EA, void* stream) {
  return comic_gru_gates_fwd(g1, S, bias, h_prev, xh, xh_ld, ru, ld_ru, xh2, xh2_ld, B, D, EA, (hipStream_t)stream);
}

int comic_op_gru_out_fwd(const float* g2, int S, const float* bias, const float* ru, int ld_ru, const float* h_prev,
                         float* cand, int ld_cand, float* y, const float* mask_out, float keep_out, const int32_t* lens,
                         int t, float* h_state, float* xh_next, int xh_ld, int B, int D, void* stream) {
  return comic_gru_out_fwd(g2, S, bias, ru, ld_ru, h_prev, cand, ld_cand, y, mask_out, keep_out, lens, t, h_state, xh_next,
                           xh_ld, B, D, (hipStream_t)stream);
}

int comic_op_gru_bwd1(const float* dy, const float* dy_part, int S, const float* mask_out, float keep_out,
                      const int32_t* lens, int t, float* dh_state, const float* ru, int ld_ru, const float* cand,
                      int ld_cand, const float* h_prev, float* dpre, int ld_dpre, int B, int D, void* stream) {
  return comic_gru_bwd1(dy, dy_part, S, mask_out, keep_out, lens, t, dh_state, ru, ld_ru, cand, ld_cand, h_prev, dpre,
                        ld_dpre, B, D, (hipStream_t)stream);
}

int comic_op_gru_bwd2(float* dxh2, int ld, const float* ru, int ld_ru, const float* h_prev, float* dpre, int ld_dpre, int B,
                      int D, int EA, void* stream) {
  return comic_gru_bwd2(dxh2, ld, ru, ld_ru, h_prev, dpre, ld_dpre, B, D, EA, (hipStream_t)stream);
}

}  // extern "C"
