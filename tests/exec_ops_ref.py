"""Float64 references of the executor-only kernel forms (tests/test_gpu_exec_ops.py), on the float32 operands.

The attention, probability and LayerNorm formulas are the oracle's own functions (oracle/decoder_ref.py), called on
float64 copies of the operands.  Where the oracle has a formula only inside a whole cell call ([x;h] K included: the
kernels start from the finished product), the few lines around the oracle's layer_norm_tf / _ln_backward / _lstm_backward
are restated here and tests/test_exec_ops_ref_cpu.py holds them to ln_lstm_cell / gru_cell / _cell_backward with an
identity matrix for K."""
import functools
import math

import numpy as np

from oracle import decoder_ref as dr
from tests import regimes

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


def attn_inputs(case, mem_rows=None, seed=None, regime=None):
    """Float32 operands of one attention step (the distribution of test_attn_step_fwd_bwd); mem_rows: rows of keys /
    values when the beams of an entry share them (mem_div).  regime (tests/regimes.py): None, ('offset', r) -- r sqrt(2) added
    to the keys, so the LayerNorm rows keys + q have a mean of r standard deviations -- or 'saturated' -- ln_g x 40.  The draws are
    those of regime None in every case."""
    B, M, D, H, Cv, method, prob, tied = case
    rng = np.random.default_rng(B * M + D + Cv if seed is None else seed)
    R = B if mem_rows is None else mem_rows
    keys = rng.standard_normal((R, M, D)).astype(np.float32)
    values = keys if tied else rng.standard_normal((R, M, Cv)).astype(np.float32)
    q = rng.standard_normal((B, D)).astype(np.float32)
    p = dict(ln_g=(1 + 0.1 * rng.standard_normal(D)).astype(np.float32),
             ln_b=(0.1 * rng.standard_normal(D)).astype(np.float32),
             v=(rng.standard_normal(D) / math.sqrt(D / H) * 3).astype(np.float32), tau=np.array(2.5, np.float32))
    if regime == 'saturated':
        p['ln_g'] = p['ln_g'] * np.float32(regimes.LN_GAIN_SCALE)
    elif regime is not None:
        assert regime[0] == 'offset', regime
        keys = regimes.offset(keys, regime[1] * math.sqrt(2.0))        # keys + q has standard deviation sqrt(2)
        values = keys if tied else values
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


def xent_operands_peaked(V, t_rows, t_stride, B, rng, lens=None):
    """The sequence-loss operands in the `peaked` regime (tests/regimes.py): logits [t_rows,B,V], lens, targets
    [B,t_stride], wmask, coef.  Batch row 0 is live at every step and holds the special rows: t = 0 all-equal, t = 1 the
    target is the arg-max, t = 2 the target's probability underflows."""
    if lens is None:
        lens = rng.integers(1, t_stride + 1, B).astype(np.int32)
        lens[:3] = (t_rows, 3, t_stride)
    assert lens[0] >= 3
    lg, tg = regimes.peaked_logits(rng, t_rows * B, V, equal_row=0, argmax_row=B, underflow_row=2 * B)
    targets = rng.integers(0, V, (B, t_stride)).astype(np.int32)
    targets[:, :t_rows] = tg.reshape(t_rows, B).T
    wmask = (np.arange(t_stride)[None, :] < lens[:, None]).astype(np.float32)
    return lg.reshape(t_rows, B, V), lens, targets, wmask, (wmask / wmask.sum()).astype(np.float32)


def dense_beam_operands(B, W, V, D, regime=None):
    """The operands of tests/test_gpu_ops.py::test_beam_step_dense_vs_oracle_step: duplicate vocabulary columns (exact ties
    in one chunk and across chunks), two beams with identical logits and totals, an entry whose other beams are at -inf, a
    finished beam, an entry with every beam finished.  regime 'peaked' (tests/regimes.py): W_o scaled so that the logits
    spread like 30 N(0,1), b_o + 200; the logits are then float64."""
    rng = np.random.default_rng(B + W + V)
    end = V - 1
    y = rng.standard_normal((B, W, D)).astype(np.float32)
    Wo = (rng.standard_normal((D, V)) / np.sqrt(D)).astype(np.float32)
    bo = (0.1 * rng.standard_normal(V)).astype(np.float32)
    Wo[:, 7] = Wo[:, 3]; bo[7] = bo[3]                          # duplicate columns: exact ties, same chunk
    Wo[:, V - 5] = Wo[:, 3]; bo[V - 5] = bo[3]                  # ... and in the last chunk
    Wo[:, 3] *= 3.0; Wo[:, 7] *= 3.0; Wo[:, V - 5] *= 3.0       # make them likely winners for some rows
    y[0, 1] = y[0, 0]                                           # two beams of entry 0 with identical logits
    lp = np.tile(np.linspace(0, -2.0, W, dtype=np.float32), (B, 1))
    lp[0, 1] = lp[0, 0]                                         # ... and equal totals: ties across beams
    lp[1, 1:] = -np.inf
    fin = np.zeros((B, W), np.int32); fin[2, 1] = 1; fin[B - 1] = 1
    lens = rng.integers(0, 5, (B, W)).astype(np.int64)
    if regime is not None:
        assert regime == 'peaked', regime
        Wo, bo = regimes.peaked_projection(Wo, bo, y.reshape(B * W, D))     # one scale: the duplicate columns stay equal
    logits = y.reshape(B * W, D).astype(np.float64) @ Wo.astype(np.float64) + bo
    logits = (logits.astype(np.float32) if regime is None else logits).reshape(B, W, V)
    return dict(end=end, y=y, Wo=Wo, bo=bo, lp=lp, fin=fin, lens=lens, logits=logits)


# ---------------------------------------------------------------------------------------------------- cells ----------
def ln_params(rng, D):
    """the ten LayerNorm vectors gamma_i, beta_i, ..., gamma_c, beta_c [10, D]"""
    ln = np.empty((10, D), np.float32)
    ln[0::2] = 1 + 0.2 * rng.standard_normal((5, D))
    ln[1::2] = 0.2 * rng.standard_normal((5, D))
    return ln


def ln_lstm_regime(g, c, ln, regime):
    """The drawn LN_LSTM operands g [S,B,4D] (split-K partials), c [B,D], ln [10,D] in a regime of tests/regimes.py.
    ('offset', r): r added to the four gate rows (their spread is 1) and to the previous cell state, with the forget
    shift + 20 so that the cell row c sigmoid(f + 1) + sigmoid(i) tanh(j) keeps the offset of c (a forget gate that varies
    along the row would cap mean / std at about 3.5).  'saturated': the five gains x 40 (pre-activations beyond +-100
    from a normalised row) and cell states to +-50."""
    g, ln = g.copy(), ln.copy()
    if regime == 'saturated':
        ln[0::2] *= np.float32(regimes.LN_GAIN_SCALE)
        return g, (None if c is None else regimes.saturate(c, regimes.CELL_PEAK)), ln
    assert regime[0] == 'offset', regime
    g[0] = regimes.offset(g[0], regime[1])
    ln[5] += np.float32(20.0)
    return g, (None if c is None else regimes.offset(c, regime[1])), ln


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


# ------------------------------------------------------------------------------------------------- whole decoder -----
# the persistent-loop geometries of the `features` regime: small-memory loops (M = 25), own-rows backward (M = 64), the
# large-memory forward loop with 1 and 4 heads a channel quarter (M = 196 and the ragged M = 130)
FEATURE_GEOMETRIES = [dict(D=512, E=256, C=2048, Cg=2048), dict(D=512, E=256, M=64),
                      dict(D=512, E=256, C=832, Cg=1024, M=196, H=4), dict(D=512, E=256, C=832, Cg=1024, M=130, H=16)]
DECODE_FEATURE_GEOMETRIES = [dict(D=512, E=256), dict()]     # greedy / beam decoding: the persistent loop, per-step launches
FEATURES_R = 32             # the target mean / std of the oracle's own z = keys + q


def features_r(geo):
    """M = 196 at four heads: shrunk to 12.  From r = 16 on the float32 oracle alone is 1.1e-4 ... 1.4e-4 off the float64 one
    in d tau / d ln_b / d W_q there (the tied values carry the offset into the softmax backward's dot products), above
    the cap of a tenth of F32_RTOL; the other geometries stay below it at 32."""
    return 12 if (geo.get('M'), geo.get('H')) == (196, 4) else FEATURES_R


def rand_lstm_params(cfg, seed):
    """dr.init_params of an add_LN LSTM decoder with non-trivial biases and LayerNorm gain / shift (the draws of
    test_gpu_path._rand_params for this cell); -> params, the generator behind them"""
    p = dr.init_params(cfg, seed)
    rng = np.random.default_rng(seed + 100)
    for k in ('b', 'b_o', 'ln_b'):
        p[k] = (0.1 * rng.standard_normal(p[k].shape)).astype(np.float32)
    p['ln_g'] = (1 + 0.1 * rng.standard_normal(p['ln_g'].shape)).astype(np.float32)
    return p, rng


SCORE_CHUNK = 112           # vocabulary columns of a workgroup of the streaming projection (csrc/beam_pack.h)
SCORE_PEAKED_GEOMETRIES = dict(V258=dict(D=512, E=256, C=2048, Cg=2048),
                               V4099=dict(D=512, E=256, C=2048, Cg=2048, token_type='word', V=4099, start_id=4097, end_id=4098))


@functools.lru_cache(maxsize=None)
def score_peaked_case(name, B=2, L=8, lens=(6, 2)):
    """Operands of tests/test_gpu_score.py::test_score_peaked_logits, built once for the GPU test and for the cap check of
    tests/test_regimes_cpu.py: COMIC-256 at the radix vocabulary or at a word vocabulary of 4099 (37 chunks of the streaming
    projection; targets in the last column of chunk 0, the first of chunk 1 and column 0), B = 2 captions of 6 and 2
    tokens.  The output projection is in the `peaked` regime of tests/regimes.py: W_o scaled so that the float64 oracle's
    logits spread like 30 N(0,1) over the live steps (the teacher-forced y do not depend on W_o), b_o + 200.
    -> geometry, cfg, float32 params, fm, im, captions, the float64 forward pass."""
    g = dict(dict(V=258, H=8, M=25, token_type='radix', start_id=256, end_id=257), **SCORE_PEAKED_GEOMETRIES[name])
    cfg = dr.DecoderConfig(rnn_size=g['D'], rnn_word_size=g['E'], attn_num_heads=g['H'], softmax_size=g['V'],
                           fm_channels=g['C'], im_embed_size=g['Cg'], token_type=g['token_type'], start_id=g['start_id'],
                           end_id=g['end_id'], l2_decay=0.0)
    p, rng = rand_lstm_params(cfg, 5)
    fm = rng.standard_normal((B, g['M'], g['C'])).astype(np.float32)
    im = rng.standard_normal((B, g['Cg'])).astype(np.float32)
    caps = np.full((B, L), -1, np.int64)
    for b in range(B):
        caps[b, 0], caps[b, 1 + lens[b]] = cfg.start_id, cfg.end_id
        caps[b, 1:1 + lens[b]] = rng.integers(0, g['V'] - 2, lens[b])
    if g['V'] > 4096:
        caps[0, 1], caps[0, 2], caps[1, 1] = SCORE_CHUNK - 1, SCORE_CHUNK, 0

    def forward(q):
        return dr.train_forward({k: f64(v) for k, v in q.items()}, cfg, f64(fm), f64(im), caps, None, None)

    out = forward(p)
    spread = float((out['logits'] - p['b_o'])[out['cache']['wmask'] > 0].std())
    p = dict(p, W_o=(p['W_o'] * (regimes.LOGIT_SCALE / spread)).astype(np.float32),
             b_o=(p['b_o'] + regimes.LOGIT_SHIFT).astype(np.float32))
    return dict(geo=g, cfg=cfg, p=p, fm=fm, im=im, caps=caps, out=forward(p))


def log_softmax_at(logits, targets, wmask):
    """[B,T,V] -> log_softmax gathered at targets [B,T], times the mask, in float64"""
    x = np.asarray(logits, np.float64)
    m = x.max(axis=-1, keepdims=True)
    lse = m[..., 0] + np.log(np.exp(x - m).sum(axis=-1))
    return (np.take_along_axis(x, targets[..., None].astype(np.int64), -1)[..., 0] - lse) * wmask


def features_cfg(geo):
    g = dict(dict(D=128, E=64, V=258, C=192, Cg=192, H=8, M=25), **geo)
    cfg = dr.DecoderConfig(rnn_size=g['D'], rnn_word_size=g['E'], attn_num_heads=g['H'], softmax_size=g['V'],
                           fm_channels=g['C'], im_embed_size=g['Cg'], l2_decay=0.0)
    return g, cfg


def z_ratio(out):
    """median |mean| / std over D of the oracle's LayerNorm input z = keys + q, live rows of every step"""
    lens = out['cache']['lens']
    return float(np.median(np.concatenate([regimes.row_ratio(st['att_cache']['z'])[t < lens].ravel()
                                           for t, st in enumerate(out['cache']['steps'])])))


@functools.lru_cache(maxsize=None)
def _features_case(geo_items, r, B, Lc, seed):
    return _features_build(dict(geo_items), r, B, Lc, seed)


def features_case(geo, r=None, B=6, Lc=11, seed=3):
    """cached: the float64 forward pass is shared by the tests of one geometry and left unchanged"""
    return _features_case(tuple(sorted(geo.items())), features_r(geo) if r is None else r, B, Lc, seed)


def _features_build(geo, r, B, Lc, seed):
    """Operands of one teacher-forced step in the `features` regime (tests/regimes.py): -> cfg, float32 params, fm, im,
    captions and the float64 oracle's forward and backward pass on them.  W_m (and an independent W_v) get delta 1 1^T with delta solved
    so that the float64 oracle's z reaches mean / std = r."""
    g, cfg = features_cfg(geo)
    p, rng = rand_lstm_params(cfg, seed)
    fm, im = regimes.features_batch(rng, B, g['M'], g['C'], g['Cg'])
    caps = np.full((B, Lc), -1, np.int64)
    for b in range(B):
        n = Lc - 2 if b == 0 else int(rng.integers(1, Lc - 1))
        caps[b, 0], caps[b, 1 + n] = cfg.start_id, cfg.end_id
        caps[b, 1:1 + n] = rng.integers(0, 256, n)
    W_m, W_v = p['W_m'], p.get('W_v')

    def with_delta(delta):
        q = dict(p, W_m=regimes.rank_one(W_m, delta))
        if W_v is not None:
            q['W_v'] = regimes.rank_one(W_v, delta)
        return q

    def forward(delta):
        return dr.train_forward({k: f64(v) for k, v in with_delta(delta).items()}, cfg, f64(fm), f64(im), caps)

    delta = regimes.solve_delta(lambda d: z_ratio(forward(d)), r, r * 1.5 / (regimes.HALF_NORMAL_MEAN * g['C']))
    p, out = with_delta(delta), forward(delta)
    grads, dfm, dim = dr.train_backward({k: f64(v) for k, v in p.items()}, cfg, out)
    return dict(cfg=cfg, geo=g, p=p, fm=fm, im=im, caps=caps, delta=delta, out=out, grads=grads, dfm=dfm, dim=dim)
