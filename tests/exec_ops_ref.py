"""Float64 references of the executor-only kernel forms (tests/test_gpu_exec_ops.py), on the float32 operands.

The attention, probability and LayerNorm formulas are the oracle's own functions (oracle/decoder_ref.py), called on
float64 copies of the operands.  Where the oracle has a formula only inside a whole cell call ([x;h] K included: the
kernels start from the finished product), the few lines around the oracle's layer_norm_tf / _ln_backward / _lstm_backward
are restated here and tests/test_exec_ops_ref_cpu.py holds them to ln_lstm_cell / gru_cell / _cell_backward with an
identity matrix for K."""
import math

import numpy as np

from oracle import decoder_ref as dr

# the bars of the op tests (the existing op tests of the same kernels); the float32 oracle alone may use a quarter
ATTN_FWD_TOL, GATES_TOL, XENT_TOL, SUM_TOL = 1e-4, 1e-5, 1e-5, 1e-5

# B, M, D, H, Cv, method, prob, tied -> workgroups per batch row of the split form
SPLIT_CASES = [
    ((3, 49, 512, 8, 512, 'add_LN', 'softmax', True), 8),       # the eighth share is empty
    ((3, 57, 128, 4, 832, 'add_LN', 'sigmoid', False), 8),      # last share one row; CW = 104
    ((40, 196, 512, 8, 512, 'add_LN', 'softmax', True), 7),
    ((64, 130, 64, 2, 192, 'dot', 'softmax', False), 4),        # ragged shares
    ((86, 64, 64, 16, 64, 'dot', 'softmax', True), 3),          # CW = 22, ragged
    ((128, 50, 64, 1, 2048, 'dot', 'sigmoid', False), 2)]       # CW = 1024, G = 1
PREFETCH_CASES = [(2, 28, 512, 8, 2048, 'add_LN', 'softmax', False), (2, 29, 512, 8, 2048, 'add_LN', 'softmax', False)]
HOLE_CASE = (128, 49, 64, 1, 4096, 'dot', 'softmax', False)
EPILOGUE_CASES = [(5, 25, 128, 4, 128, 'add_LN', 'softmax', True), SPLIT_CASES[0][0]]
BWD_CASES = [(c, s) for c, s in SPLIT_CASES if c[4] < 2048] + [((5, 25, 512, 8, 512, 'add_LN', 'softmax', True), 1)]
LN_LSTM_D = [64, 100, 256, 320, 512, 576, 1024, 2048]
GRU_D = [64, 100, 256, 320, 512, 576, 1024]


def f64(x):
    return None if x is None else np.asarray(x, np.float64)


def attn_cfg(case):
    B, M, D, H, Cv, method, prob, tied = case
    return dr.DecoderConfig(rnn_size=D, attn_num_heads=H, attn_alignment_method=method, attn_probability_fn=prob,
                            cnn_fm_projection='tied' if tied else 'independent')


def attn_inputs(case, mem_rows=None, seed=None):
    """Float32 operands of one attention step (the distribution of test_attn_step_fwd_bwd); mem_rows: rows of keys /
    values when the beams of an entry share them (mem_div)."""
    B, M, D, H, Cv, method, prob, tied = case
    rng = np.random.default_rng(B * M + D + Cv if seed is None else seed)
    R = B if mem_rows is None else mem_rows
    keys = rng.standard_normal((R, M, D)).astype(np.float32)
    values = keys if tied else rng.standard_normal((R, M, Cv)).astype(np.float32)
    q = rng.standard_normal((B, D)).astype(np.float32)
    p = dict(ln_g=(1 + 0.1 * rng.standard_normal(D)).astype(np.float32),
             ln_b=(0.1 * rng.standard_normal(D)).astype(np.float32),
             v=(rng.standard_normal(D) / math.sqrt(D / H) * 3).astype(np.float32), tau=np.array(2.5, np.float32))
    return dict(keys=keys, values=values, q=q, p=p, rng=rng)


def mem_repeat(x, W):
    """mem_div = W: batch row b attends to memory row b // W."""
    return np.repeat(x, W, axis=0)


def attn_fwd_ref(case, keys, values, q, p, mask, keep, dtype=np.float64):
    """-> alpha, alpha_d [B,H,M], ctx [B,Cv], the oracle's score cache."""
    cfg = attn_cfg(case)
    cast = (lambda x: None if x is None else np.asarray(x, dtype))
    pp = {k: cast(v) for k, v in p.items()}
    alpha, ac = dr.attention_scores(pp, cfg, cast(keys), cast(q))
    alpha_d = dr.dropout(alpha, cast(mask), keep)
    return alpha, alpha_d, dr.context(cfg, alpha_d, cast(values)), ac


def epilogue_ref(ctx, att_prev, lens, t, mask_next, keep_in):
    """impute_finished select of the attention state and the next step's dropped LSTM input columns."""
    fin = (t >= np.asarray(lens))[:, None]
    att_next = np.where(fin, att_prev, ctx)
    return att_next, dr.dropout(att_next, mask_next, keep_in)


def attn_bwd_ref(case, keys, values, q, p, mask, keep, dctx, dmap, lens=None, t=0, dtype=np.float64):
    """Per-row backward of one attention step: dq [B,D], dkeys [B,M,D], dvalues [B,M,Cv] (tied: add both) and the
    parameter-gradient rows pgrad [B, 3D+1] = d v | d ln_g | d ln_b | d tau of each batch row.  Finished rows
    (t >= lens[b]) kept their previous attention state: no d ctx passes, the map-loss term dmap still does."""
    B, M, D, H, Cv, method, prob, tied = case
    cfg = attn_cfg(case)
    cast = (lambda x: None if x is None else np.asarray(x, dtype))
    keys, values, q, mask, dctx, dmap = (cast(x) for x in (keys, values, q, mask, dctx, dmap))
    pp = {k: cast(v) for k, v in p.items()}
    live = np.ones((B, 1), dtype) if lens is None else (t < np.asarray(lens))[:, None].astype(dtype)
    dcl = (dctx * live).reshape(B, H, Cv // H)
    alpha, alpha_d, _, _ = attn_fwd_ref(case, keys, values, q, pp, mask, keep, dtype)
    dalpha_d = np.einsum('bhd,bmhd->bhm', dcl, values.reshape(B, M, H, Cv // H))
    if dmap is not None:
        dalpha_d = dalpha_d + dmap[:, None, :]
    dvalues = np.einsum('bhm,bhd->bmhd', alpha_d, dcl).reshape(B, M, Cv)
    dalpha = dr.dropout(dalpha_d, mask, keep)
    dq = np.zeros((B, D), dtype)
    dkeys = np.zeros((B, M, D), dtype)
    pgrad = np.zeros((B, 3 * D + 1), dtype)
    for b in range(B):          # row by row: the oracle sums its parameter gradients over the batch
        g = {k: np.zeros_like(v) for k, v in pp.items()}
        a_b, ac = dr.attention_scores(pp, cfg, keys[b:b + 1], q[b:b + 1])
        dkeys[b:b + 1], dq[b:b + 1] = dr._attention_backward(pp, cfg, keys[b:b + 1], q[b:b + 1], ac, a_b, dalpha[b:b + 1], g)
        if method == 'add_LN':
            pgrad[b] = np.concatenate([g['v'], g['ln_g'], g['ln_b'], np.reshape(g['tau'], 1)])
    return dict(dq=dq, dkeys=dkeys, dvalues=dvalues, pgrad=pgrad)


def map_loss_ref(hist, scale):
    """hist [Tp,B,H,M] -> mean((1 - sum_h hist)^2) * scale and its gradient d / d (sum_h hist) [Tp,B,M]."""
    flat = f64(hist).sum(axis=2)
    return ((1.0 - flat) ** 2).mean() * scale, 2.0 * (flat - 1.0) / flat.size * scale


def xent_ref(logits, targets_bt, coef_bt, wmask_bt, lens):
    """Sequence loss rows of time-major logits [T,B,V] against [B,Ts] tables (Ts >= T), as test_xent_fwd_bwd:
    -> zeroed logits, loss rows [T,B], d logits [T,B,V], arg-max ids."""
    T = logits.shape[0]
    live = np.arange(T)[:, None] < np.asarray(lens)[None, :]
    lg = logits * live[..., None]
    lsm = dr.log_softmax(lg.astype(np.float64), -1)
    tg = targets_bt[:, :T].T[..., None]
    xent = -np.take_along_axis(lsm, tg, 2)[..., 0] * wmask_bt[:, :T].T
    oh = np.zeros_like(lsm)
    np.put_along_axis(oh, tg, 1.0, 2)
    return lg, xent, (np.exp(lsm) - oh) * coef_bt[:, :T].T[..., None], lg.argmax(-1)


# ---------------------------------------------------------------------------------------------------- cells ----------
def ln_params(rng, D):
    """the ten LayerNorm vectors gamma_i, beta_i, ..., gamma_c, beta_c [10, D]"""
    ln = np.empty((10, D), np.float32)
    ln[0::2] = 1 + 0.2 * rng.standard_normal((5, D))
    ln[1::2] = 0.2 * rng.standard_normal((5, D))
    return ln


def ln_lstm_fwd_ref(g, ln, c_prev, dtype=np.float64):
    """dr.ln_lstm_cell from the finished product g [B,4D] on: -> gates_act [B,4D], xhat [B,5D], rstd [B,5], c_new, h_new."""
    g, ln = np.asarray(g, dtype), np.asarray(ln, dtype)
    D = g.shape[1] // 4
    c = np.zeros((g.shape[0], D), dtype) if c_prev is None else np.asarray(c_prev, dtype)
    pre, xh, rs = [], [], []
    for k in range(4):
        z = g[:, k * D:(k + 1) * D]
        y, mean, rstd = dr.layer_norm_tf(z, ln[2 * k], ln[2 * k + 1])
        pre.append(y); xh.append((z - mean) * rstd); rs.append(rstd)
    si, tj, sf, so = dr.sigmoid(pre[0]), np.tanh(pre[1]), dr.sigmoid(pre[2] + 1.0), dr.sigmoid(pre[3])
    craw = c * sf + si * tj
    c2, mean, rstd = dr.layer_norm_tf(craw, ln[8], ln[9])
    xh.append((craw - mean) * rstd); rs.append(rstd)
    return dict(gates_act=np.concatenate([si, tj, sf, so], 1), xhat=np.concatenate(xh, 1), rstd=np.concatenate(rs, 1),
                c_new=c2, h_new=np.tanh(c2) * so)


def ln_lstm_bwd_ref(fw, ln, c_prev, dc2, dh2, dtype=np.float64):
    """The LN_LSTM branch of dr._cell_backward without the products: -> dg [B,4D], the ten per-row gradient rows
    [B,10,D] (order of `ln`), d c_prev."""
    ln = np.asarray(ln, dtype)
    D = ln.shape[1]
    ga, xhat, rs = fw['gates_act'], fw['xhat'], fw['rstd']
    si, tj, sf, so = (ga[:, k * D:(k + 1) * D] for k in range(4))
    xh = [xhat[:, k * D:(k + 1) * D] for k in range(5)]
    c = np.zeros_like(si) if c_prev is None else np.asarray(c_prev, dtype)
    tc = np.tanh(fw['c_new'])
    rows = np.zeros((si.shape[0], 10, D), dtype)
    dso = dh2 * tc
    dcn = dc2 + dh2 * so * (1 - tc * tc)
    dcraw, _, _ = dr._ln_backward(dcn, xh[4], rs[:, 4:5], ln[8])
    rows[:, 8], rows[:, 9] = dcn * xh[4], dcn
    dpre = [dcraw * tj * si * (1 - si), dcraw * si * (1 - tj * tj), dcraw * c * sf * (1 - sf), dso * so * (1 - so)]
    dz = []
    for k in range(4):
        z, _, _ = dr._ln_backward(dpre[k], xh[k], rs[:, k:k + 1], ln[2 * k])
        rows[:, 2 * k], rows[:, 2 * k + 1] = dpre[k] * xh[k], dpre[k]
        dz.append(z)
    return np.concatenate(dz, 1), rows, dcraw * sf


def gru_fwd_ref(g1, b_g, g2_of, b_c, h_prev, dtype=np.float64):
    """dr.gru_cell from the finished products on.  g1 [B,2D]; g2_of(r*h) -> the candidate product [B,D] (it depends on
    r); -> r, u, cand, h_new."""
    g1 = np.asarray(g1, dtype)
    D = g1.shape[1] // 2
    h = np.zeros((g1.shape[0], D), dtype) if h_prev is None else np.asarray(h_prev, dtype)
    ru = dr.sigmoid(g1 + np.asarray(b_g, dtype))
    r, u = ru[:, :D], ru[:, D:]
    cand = np.tanh(np.asarray(g2_of(r * h), dtype) + np.asarray(b_c, dtype))
    return r, u, cand, u * h + (1 - u) * cand


def gru_bwd_ref(r, u, cand, h_prev, dh2, drh):
    """The GRU branch of dr._cell_backward without the products: d cand_pre, d u_pre, d r_pre, and the shares of
    d h_prev that do not pass through a product: dh2*u and drh*r."""
    return dh2 * (1 - u) * (1 - cand * cand), dh2 * (h_prev - cand) * u * (1 - u), drh * h_prev * r * (1 - r), dh2 * u, drh * r


def state_select(fin, prev, new):
    prev = np.zeros_like(new) if prev is None else prev
    return np.where(np.asarray(fin)[:, None], prev, new)
