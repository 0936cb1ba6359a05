// Op-level C entries of the executor-only kernel forms (include/comic_hip.h, "op-level entries of the executor-only
// forms"): each forwards its arguments to the internal entry of exec_entries.h and does nothing else, so a test can put
// one form on its own operands; the entries of the fused step kernels first pack the weights as the executors do once
// per call.  No product code calls these.
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

// ---- the fused LSTM step kernels (decoder_fused.hip) on the raw parameters: pack the panel the executors pack once per
// call (panel_floats: comic_lstm_panel_floats of the shape, checked), then the host function they call per step.
namespace {
struct OpStopScope {          // the decode loops' stop word for the launches of one entry, as the executors scope it
  OpStopScope(const int32_t* stop, int t) {
    g_comic_stop.p = stop;
    g_comic_stop.t = t;
  }
  ~OpStopScope() { g_comic_stop = ComicStop(); }
};
}  // namespace

int comic_op_lstm_step_fused(const float* K, float* panel, int64_t panel_floats, const float* xh, int ld_xh,
                             const float* bias, const float* c_prev, const float* h_prev, float* gates_act, float* c_new,
                             float* y, const float* mask_out, float keep_out, const int32_t* lens, int t, float* c_state,
                             float* h_state, float* xh_next, int xh_ld, int B, int D, int Wd, const int32_t* stop,
                             int stop_t, void* stream) {
  COMIC_REQUIRE(K && panel && D > 0 && Wd > 0 && comic_fused_step_supported(D, Wd), "op_lstm_step_fused: unsupported shape (D %d, Wd %d)", D, Wd);
  COMIC_REQUIRE(panel_floats >= comic_lstm_panel_floats(D, Wd, 0), "op_lstm_step_fused: panel too small");
  hipStream_t st = (hipStream_t)stream;
  int rc = comic_pack_lstm_panels(K, panel, nullptr, D, Wd, st);
  if (rc) return rc;
  OpStopScope stop_scope(stop, stop_t);
  return comic_lstm_step_fused(xh, ld_xh, panel, bias, c_prev, h_prev, gates_act, c_new, y, mask_out, keep_out, lens, t,
                               c_state, h_state, xh_next, xh_ld, B, D, Wd, st);
}

int comic_op_input_grad_fused(const float* K, float* panel, int64_t panel_floats, const float* dg, const float* mask,
                              float keep, float* demb, float* datt, float* dh, const int32_t* lens, int t, int carry, int B,
                              int E, int A, int D, void* stream) {
  COMIC_REQUIRE(K && panel && D > 0 && E >= 0 && A >= 0 && comic_fused_step_supported(D, E + A + D),
                "op_input_grad_fused: unsupported shape (D %d, E %d, A %d)", D, E, A);
  COMIC_REQUIRE(panel_floats >= comic_lstm_panel_floats(D, E + A + D, 1), "op_input_grad_fused: panel too small");
  hipStream_t st = (hipStream_t)stream;
  int rc = comic_pack_lstm_panels(K, nullptr, panel, D, E + A + D, st);
  if (rc) return rc;
  return comic_input_grad_fused(dg, panel, mask, keep, demb, datt, dh, lens, t, carry, B, E, A, D, st);
}

int comic_op_lstm_grad_fused(const float* W_q, float* panel, int64_t panel_floats, const float* dq, const float* gates_act,
                             const float* c_prev, const float* c_new, const float* dy, const float* mask_out,
                             float keep_out, const int32_t* lens, int t, float* dc_state, float* dh_state, float* dg, int B,
                             int D, void* stream) {
  COMIC_REQUIRE(D > 0 && panel_floats >= (int64_t)D * D, "op_lstm_grad_fused: panel too small");
  hipStream_t st = (hipStream_t)stream;
  int rc = comic_pack_wq_panel(W_q, panel, D, st);        // refuses D % 16 != 0, as the step itself does
  if (rc) return rc;
  return comic_lstm_grad_fused(dq, panel, gates_act, c_prev, c_new, dy, mask_out, keep_out, lens, t, dc_state, dh_state,
                               dg, B, D, st);
}

}  // extern "C"
