"""The operand regimes of tests/regimes.py, checked without a GPU: each generator holds what it claims (measured on the
float64 reference's intermediates), the float64 references and their float32 restatements are finite there, the
restatement's error stays under the cap at which a GPU test would stop discriminating (a quarter of the op bar, a tenth of
the step bar F32_RTOL for whole-decoder tests), regime None reproduces the draws of the normal tests bit for bit, and a
reference restated with each of the six shortcuts of the regimes' table lands outside the bar in its regime.
Every figure is printed (pytest -s): regime statistic, restatement error, bar."""
import math

import numpy as np
import pytest

from oracle import decoder_ref as dr
from tests import exec_ops_ref as R
from tests import regimes as G
from tests import step_ops_ref as S

F32_RTOL = 1e-3             # tests/gpu_util.py (which imports torch and the library: not here)
# Every operand below comes from the builder the GPU test of the same case uses (exec_ops_ref, step_ops_ref, regimes), at the
# same shapes and seeds: the GPU tests take their op's normal bar on the strength of the caps asserted here.
ATTN_REGIMES = [('offset', 4), ('offset', 32), 'saturated']
# the cases of the GPU tests: test_attn_step_fwd_bwd's first add_LN case (also the smallest add_LN softmax case of
# test_attn_bwd_forms), the two smallest add_LN entries of SPLIT_CASES, the small EPILOGUE_CASES entry, the add_LN mem_div case
ATTN_CASES = [(5, 25, 512, 8, 512, 'add_LN', 'softmax', True), R.SPLIT_CASES[0][0], R.SPLIT_CASES[1][0], R.EPILOGUE_CASES[0],
              (9, 25, 512, 8, 2048, 'add_LN', 'softmax', False)]


def report(name, regime, stat, err, op_bar, cap_share=0.25):
    b = G.bar(op_bar, err)
    print('  %-34s %-14s statistic %-9.4g float32 restatement %.2e  cap %.2e  bar %.1e' % (name, regime, stat, err,
                                                                                           cap_share * op_bar, b))
    assert np.isfinite(err) and err <= cap_share * op_bar, (name, regime, err)
    assert b == op_bar
    return b


def all_finite(*trees):
    for t in trees:
        for v in (t.values() if isinstance(t, dict) else t):
            if isinstance(v, np.ndarray):
                assert np.isfinite(v).all()


def partials(rng, n, *shape):
    return (rng.standard_normal((n,) + shape) / np.sqrt(n)).astype(np.float32)


# ------------------------------------------------------------------------------------------ regime None -------------
def test_regime_none_reproduces_the_draws_of_the_normal_tests():
    """attn_inputs / step_inputs restated as they were before they took `regime`: the same arrays, bit for bit"""
    for case in ATTN_CASES + [R.SPLIT_CASES[3][0]]:
        B, M, D, H, Cv, method, prob, tied = case
        rng = np.random.default_rng(B * M + D + Cv)
        keys = rng.standard_normal((B, M, D)).astype(np.float32)
        values = keys if tied else rng.standard_normal((B, M, Cv)).astype(np.float32)
        q = rng.standard_normal((B, D)).astype(np.float32)
        p = dict(ln_g=(1 + 0.1 * rng.standard_normal(D)).astype(np.float32),
                 ln_b=(0.1 * rng.standard_normal(D)).astype(np.float32),
                 v=(rng.standard_normal(D) / math.sqrt(D / H) * 3).astype(np.float32), tau=np.array(2.5, np.float32))
        for got in (R.attn_inputs(case), R.attn_inputs(case, regime=None)):
            for k, want in (('keys', keys), ('values', values), ('q', q)):
                np.testing.assert_array_equal(got[k], want)
            for k in p:
                np.testing.assert_array_equal(got['p'][k], p[k])
        # the generator is left where it was: the masks drawn from it afterwards are the same too
        assert R.attn_inputs(case)['rng'].random() == rng.random()
    for B, D, EA in S.FUSED_SHAPES[:3]:
        Wd = EA + D
        rng = np.random.default_rng(1000 * B + D + EA)
        want = dict(K=(rng.standard_normal((Wd, 4 * D)) / np.sqrt(Wd)).astype(np.float32), b=S.gate_bias(rng, D),
                    xh=rng.standard_normal((B, Wd)).astype(np.float32), c=rng.standard_normal((B, D)).astype(np.float32),
                    h=(0.5 * rng.standard_normal((B, D))).astype(np.float32),
                    mask=(rng.random((B, D)) < S.KEEP).astype(np.float32), lens=S.lens_for(B))
        for got in (S.step_inputs(B, D, EA), S.step_inputs(B, D, EA, regime=None)):
            assert set(got) == set(want)
            for k in want:
                np.testing.assert_array_equal(got[k], want[k])
    # the other builders: the regime changes the named operands only
    for a, b, changed in ((S.step_inputs(17, 36, 32), S.step_inputs(17, 36, 32, regime='saturated'), {'b', 'c'}),
                          (S.grad_inputs(17, 10, 22, 36), S.grad_inputs(17, 10, 22, 36, regime='saturated'), {'dg'}),
                          (S.infer_inputs(12, 3, 36, 20, 12), S.infer_inputs(12, 3, 36, 20, 12, regime='saturated'), {'b', 'c'}),
                          (S.qgrad_inputs(17, 48), S.qgrad_inputs(17, 48, regime='saturated'), {'gates_act', 'c_new', 'c'})):
        for k in a:
            same = a[k] is b[k] or (a[k] is not None and np.array_equal(a[k], b[k]))
            assert same == (k not in changed), k


# ------------------------------------------------------------------------------------------ attention ---------------
def attn_operands(case, regime, mem_div=1):
    B, M, D, H, Cv = case[:5]
    inp = R.attn_inputs(case, mem_rows=B // mem_div if mem_div > 1 else None, regime=regime)
    mask = (inp['rng'].random((B, H, M)) < 0.9).astype(np.float32)
    keys, values = inp['keys'], inp['values']
    if mem_div > 1:
        keys, values = R.mem_repeat(keys, mem_div), R.mem_repeat(values, mem_div)
    return inp, keys, values, mask


@pytest.mark.parametrize('regime', ATTN_REGIMES, ids=str)
@pytest.mark.parametrize('case', ATTN_CASES, ids=lambda c: 'x'.join(map(str, c[:5])))
def test_attention_regimes(case, regime):
    B, M, D, H, Cv = case[:5]
    inp, keys, values, mask = attn_operands(case, regime, 3 if Cv == 2048 else 1)
    f64 = R.attn_fwd_ref(case, keys, values, inp['q'], inp['p'], mask, 0.9)
    with np.errstate(over='ignore'):
        f32 = R.attn_fwd_ref(case, keys, values, inp['q'], inp['p'], mask, 0.9, dtype=np.float32)
    ac = f64[3]
    if regime == 'saturated':
        stat = float(np.abs((ac['z'] - ac['mean']) * ac['rstd'] * inp['p']['ln_g'] + inp['p']['ln_b']).max())
        assert stat >= 89
    else:
        stat = float(np.median(G.row_ratio(ac['z'])))
        assert abs(stat / regime[1] - 1) <= 0.2
    all_finite(f64[:3], f32[:3])
    for name, a, b in zip(('alpha', 'alpha_d', 'ctx'), f32, f64):
        report('attention fwd ' + name, str(regime), stat, G.rel_err(a, b), R.ATTN_FWD_TOL)
    if Cv == 2048:
        return
    rng = np.random.default_rng(B + M + D)
    dctx = rng.standard_normal((B, Cv)).astype(np.float32)
    dmap = (0.01 * rng.standard_normal((B, M))).astype(np.float32)
    lens = np.array([3, 1, 5, 2, 9, 2, 4], np.int32)[:B]
    b64 = R.attn_bwd_ref(case, keys, values, inp['q'], inp['p'], mask, 0.9, dctx, dmap, lens, 2)
    with np.errstate(over='ignore'):
        b32 = R.attn_bwd_ref(case, keys, values, inp['q'], inp['p'], mask, 0.9, dctx, dmap, lens, 2, dtype=np.float32)
    all_finite(b64, b32)
    for k in b64:
        report('attention bwd ' + k, str(regime), stat, G.rel_err(b32[k], b64[k]), F32_RTOL)


# ------------------------------------------------------------------------------------------ cells -------------------
# offset(32) shrunk to offset(8) for the LN_LSTM forward: at r = 32 the float32 restatement is 7e-6 off on the gate
# activations (the rounding of a row at magnitude 32 against its spread of 1), 70 % of GATES_TOL; at r = 8 it is 2e-6
LN_LSTM_REGIMES = [('offset', 4), ('offset', 8), 'saturated']


@pytest.mark.parametrize('regime', LN_LSTM_REGIMES, ids=str)
@pytest.mark.parametrize('D', [128, 512])
def test_ln_lstm_regimes(D, regime):
    B, n = 5, 3
    rng = np.random.default_rng(D + n)
    g, ln = partials(rng, n, B, 4 * D), R.ln_params(rng, D)
    c = rng.standard_normal((B, D)).astype(np.float32)
    g, c, ln = R.ln_lstm_regime(g, c, ln, regime)
    gs = R.f64(g).sum(0)
    f64 = R.ln_lstm_fwd_ref(gs, ln, c)
    with np.errstate(over='ignore'):
        f32 = R.ln_lstm_fwd_ref((g[0] + g[1]) + g[2], ln, c, dtype=np.float32)
    si, tj, sf, so = (f64['gates_act'][:, k * D:(k + 1) * D] for k in range(4))
    if regime == 'saturated':
        pre = f64['xhat'][:, :4 * D].reshape(B, 4, D) * ln[0:8:2] + ln[1:8:2]
        stat = float(np.abs(pre).max())
        assert stat >= 89 and np.abs(c).max() == G.CELL_PEAK
    else:
        rows = np.concatenate([gs.reshape(B * 4, D), R.f64(c) * sf + si * tj])
        stat = float(np.median(G.row_ratio(rows)))
        assert (np.abs(G.row_ratio(rows) / regime[1] - 1) <= 0.2).all()
    all_finite(f64, f32)
    for k in f64:
        report('LN_LSTM fwd D=%d %s' % (D, k), str(regime), stat, G.rel_err(f32[k], f64[k]), R.GATES_TOL)
    fw32 = {k: v.astype(np.float32) for k, v in f64.items()}
    dc, dh = (rng.standard_normal((B, D)).astype(np.float32) for _ in range(2))
    b64 = R.ln_lstm_bwd_ref({k: R.f64(v) for k, v in fw32.items()}, ln, c, R.f64(dc), R.f64(dh))
    b32 = R.ln_lstm_bwd_ref(fw32, ln, c, dc, dh, dtype=np.float32)
    all_finite(b64, b32)
    for name, a, b in zip(('dg', 'ln rows', 'dc'), b32, b64):
        report('LN_LSTM bwd D=%d %s' % (D, name), str(regime), stat, G.rel_err(a, b), F32_RTOL)


def ln_tanh_ref(x, gamma, beta, dtype=np.float64):
    """dr.legacy_head_forward up to the product: y = tanh(LN(x) gamma + beta), xhat"""
    y, xhat = G.two_pass_layer_norm(x, gamma, beta, dtype=dtype)
    return np.tanh(y), xhat


def ln_tanh_operands(C, r, B=5):
    rng = np.random.default_rng(C + r)
    return dict(x=G.nonneg_offset(rng, (B, C), r), gamma=rng.uniform(0.5, 1.5, C).astype(np.float32),
                beta=(0.1 * rng.standard_normal(C)).astype(np.float32), dy=rng.standard_normal((B, C)).astype(np.float32))


@pytest.mark.parametrize('r', G.OFFSETS)
@pytest.mark.parametrize('C', [192, 2048])
def test_ln_tanh_regimes(C, r):
    """the legacy encoder head on non-negative rows; its bar is that of the same formula in the attention step"""
    o = ln_tanh_operands(C, r)
    assert o['x'].min() >= 0
    stat = float(np.median(G.row_ratio(o['x'])))
    assert (np.abs(G.row_ratio(o['x']) / r - 1) <= 0.2).all()
    y64, xh64 = ln_tanh_ref(o['x'], o['gamma'], o['beta'])
    y32, xh32 = ln_tanh_ref(o['x'], o['gamma'], o['beta'], np.float32)
    all_finite([y64, xh64, y32, xh32])
    report('LN_tanh C=%d y' % C, 'offset(%d)' % r, stat, G.rel_err(y32, y64), R.ATTN_FWD_TOL)
    report('LN_tanh C=%d xhat' % C, 'offset(%d)' % r, stat, G.rel_err(xh32, xh64), R.ATTN_FWD_TOL)


def gates_operands(D, regime, B=6, n=3):
    """the operands of test_lstm_gates_split_k_partials_and_bias"""
    rng = np.random.default_rng(D)
    g = partials(rng, n, B, 4 * D)
    bias = (0.1 * rng.standard_normal(4 * D)).astype(np.float32)
    c = rng.standard_normal((B, D)).astype(np.float32)
    if regime == 'saturated':
        g = G.saturate_partials(g, bias)
        c = G.saturate(c, G.CELL_PEAK)
    return rng, g, bias, c


def test_saturated_gate_operands():
    D = 128
    rng, g, bias, c = gates_operands(D, 'saturated')
    gs = R.f64(g).sum(0) + bias
    stat = float(np.abs(gs).max())
    assert stat >= 89 and np.abs(c).max() == G.CELL_PEAK
    f64 = S.lstm_step_ref(None, None, None, c, None, None, 1.0, None, 0, g=gs)
    with np.errstate(over='ignore'):
        f32 = S.lstm_step_ref(None, None, None, c, None, None, 1.0, None, 0, np.float32, g=((g[0] + g[1]) + g[2]) + bias)
    all_finite(f64, f32)
    for k in ('gates_act', 'c_new', 'h_new'):
        report('LSTM gates ' + k, 'saturated', stat, G.rel_err(f32[k], f64[k]), R.GATES_TOL)
    assert np.abs(f64['c_new']).max() > 40 and np.abs(np.tanh(f64['c_new'])).max() == 1.0      # tanh(c) saturates
    # GRU: the smallest test_gru_kernels case
    D, n, B = 64, 1, 5
    rng = np.random.default_rng(D + 256 + n)
    g1, g2 = G.saturate_partials(partials(rng, n, B, 2 * D)), G.saturate_partials(partials(rng, n, B, D))
    b_g = (1 + 0.1 * rng.standard_normal(2 * D)).astype(np.float32)
    b_c = (0.1 * rng.standard_normal(D)).astype(np.float32)
    h = rng.standard_normal((B, D)).astype(np.float32)
    assert np.abs(R.f64(g1).sum(0) + b_g).max() >= 89 and np.abs(R.f64(g2).sum(0) + b_c).max() >= 89
    f64 = R.gru_fwd_ref(R.f64(g1).sum(0), b_g, lambda rh: R.f64(g2).sum(0), b_c, h)
    with np.errstate(over='ignore'):
        f32 = R.gru_fwd_ref(g1[0], b_g, lambda rh: g2[0], b_c, h, dtype=np.float32)
    all_finite(f64, f32)
    for name, a, b in zip(('r', 'u', 'cand', 'h_new'), f32, f64):
        report('GRU ' + name, 'saturated', float(np.abs(g1).max()), G.rel_err(a, b), R.GATES_TOL)


@pytest.mark.parametrize('shape', S.FUSED_SHAPES[:2], ids=str)
def test_saturated_step_operands(shape):
    B, D, EA = shape
    inp = S.step_inputs(B, D, EA, regime='saturated')
    g = R.f64(inp['xh']) @ R.f64(inp['K']) + inp['b']
    stat = float(np.abs(g).max())
    assert stat >= 89 and np.abs(inp['c']).max() == G.CELL_PEAK
    args = (inp['xh'], inp['K'], inp['b'], inp['c'], inp['h'], inp['mask'], S.KEEP, inp['lens'], S.T_STEP)
    f64 = S.lstm_step_ref(*args)
    with np.errstate(over='ignore'):
        f32 = S.lstm_step_ref(*args, dtype=np.float32)
    all_finite(f64, f32)
    for k in f64:
        report('fused step %s %s' % (shape, k), 'saturated', stat, S.figure(f32[k], f64[k]), S.GATES_TOL)


@pytest.mark.parametrize('shape', S.QGRAD_SHAPES[:2], ids=str)
def test_saturated_step_gradient_operands(shape):
    q = S.qgrad_inputs(*shape, regime='saturated')
    args = (q['dq'], q['Wq'], q['gates_act'], q['c'], q['c_new'], q['dy'], q['mask'], S.KEEP, q['lens'], S.T_STEP, q['dc'], q['dh'])
    f64, f32 = S.lstm_grad_ref(*args), S.lstm_grad_ref(*args, dtype=np.float32)
    all_finite(f64, f32)
    zeros = float(np.mean(f64['dg'] == 0))
    assert zeros > 0.3                          # s (1 - s) underflows: mostly exact zeros
    for k in ('dg', 'dc'):
        report('fused gate gradient %s %s' % (shape, k), 'saturated', zeros, S.figure(f32[k], f64[k]), S.GATES_TOL)


@pytest.mark.parametrize('shape', S.GRAD_SHAPES[:2], ids=str)
def test_saturated_input_gradient_operands(shape):
    B, E, A, D = shape
    i = S.grad_inputs(*shape, regime='saturated')
    args = (i['dg'], i['K'], i['mask'], S.KEEP, i['datt'], i['dh'], i['lens'], S.T_STEP, 1, E, A)
    f64, f32 = S.input_grad_ref(*args), S.input_grad_ref(*args, dtype=np.float32)
    all_finite(f64, f32)
    zeros = float(np.mean(i['dg'] == 0))
    assert zeros > 0.6
    for k in f64:
        report('fused input gradient %s %s' % (shape, k), 'saturated', zeros, S.figure(f32[k], f64[k]), S.GATES_TOL)


@pytest.mark.parametrize('shape,emulate', [(S.INFER_FUSED_SHAPES[0], False), (S.STREAM_SHAPES[0][0], True), (S.BOTH_SHAPE, True),
                                           (S.BOTH_SHAPE, False)], ids=str)
def test_saturated_decode_step_operands(shape, emulate):
    """the fused path against plain float32, the streaming path against the emulation of its bf16 hi / lo arithmetic"""
    R_, W, D, E, A = shape
    inp = S.infer_inputs(R_, W, D, E, A, regime='saturated')
    x, c_in, f64 = S.infer_step_ref(inp, W)
    stat = float(np.abs(R.f64(x) @ R.f64(inp['K']) + inp['b']).max())
    assert stat >= 89 and np.abs(inp['c']).max() == G.CELL_PEAK
    with np.errstate(over='ignore'):
        f32 = S.infer_step_ref(inp, W, emulate=True)[2] if emulate else \
            S.lstm_step_ref(x, inp['K'], inp['b'], c_in, None, None, 1.0, None, 0, np.float32)
    all_finite(f64, f32)
    for k in ('c_state', 'h_state', 'y'):
        report('decode step %s %s %s' % (shape, 'stream' if emulate else 'fused', k), 'saturated', stat,
               S.figure(f32[k], f64[k]), S.STREAM_TOL if emulate else S.GATES_TOL)


# ------------------------------------------------------------------------------------------ losses ------------------
def test_peaked_loss_operands():
    for V in (258, 25599):
        ops = R.xent_operands_peaked(V, 7, 7, 5, np.random.default_rng(V), lens=np.array([7, 3, 5, 1, 6], np.int32))
        logits, lens, targets, wmask, coef = ops
        T, B = logits.shape[:2]
        lead = G.top1_lead(logits.reshape(T * B, V))
        stat = float(np.mean(lead > 20))
        assert stat >= 0.9
        lg, xent, dl, amax = R.xent_ref(*ops[:1], targets, coef, wmask, lens)
        lsm32 = dr.log_softmax(lg.astype(np.float32), -1)
        x32 = -np.take_along_axis(lsm32, targets[:, :T].T[..., None], 2)[..., 0] * wmask[:, :T].T
        assert np.isfinite(xent).all() and np.isfinite(dl).all() and np.isfinite(x32).all()
        assert (logits[0, 0] == logits[0, 0, 0]).all() and amax[0, 0] == 0 and abs(xent[0, 0] - math.log(V)) < 1e-9
        assert 0 <= xent[1, 0] < np.finfo(np.float32).eps and amax[1, 0] == targets[0, 1]
        assert logits[2, 0].max() - logits[2, 0, targets[0, 2]] > 100 and abs(xent[2, 0] - 150) < 1e-3
        assert xent.max() > 100 and np.abs(logits).max() > 200
        report('xent rows V=%d' % V, 'peaked', stat, S.figure(x32, xent), R.XENT_TOL)
        oh = np.zeros_like(lsm32)
        np.put_along_axis(oh, targets[:, :T].T[..., None].astype(np.int64), 1.0, 2)
        report('xent d logits V=%d' % V, 'peaked', stat, G.rel_err((np.exp(lsm32) - oh) * coef[:, :T].T[..., None], dl), R.XENT_TOL)


@pytest.mark.parametrize('shape', [(4, 3, 258, 128), (4, 3, 2500, 96), (5, 8, 9000, 128)], ids=str)
def test_peaked_beam_step_operands(shape):
    """the operands of test_beam_step_dense_peaked_logits: the scores of the float64 step's top W through a float32 product
    and log-softmax, against the bar of the sibling's scores"""
    B, W, V, D = shape
    o = R.dense_beam_operands(B, W, V, D, 'peaked')
    logits = o['logits']
    assert logits.dtype == np.float64 and np.abs(logits).max() > 250
    assert abs((logits - o['bo']).std() / G.LOGIT_SCALE - 1) < 0.01
    assert (o['Wo'][:, 7] == o['Wo'][:, 3]).all() and o['bo'][7] == o['bo'][3]
    lg32 = (o['y'].reshape(B * W, D) @ o['Wo'] + o['bo']).reshape(B, W, V)
    assert lg32.dtype == np.float32
    live = o['fin'] == 0
    tot64 = (o['lp'][:, :, None] + dr.log_softmax(logits, -1))[live]
    tot32 = (o['lp'][:, :, None] + dr.log_softmax(lg32, -1))[live]
    top = np.argsort(-tot64, -1)[:, :W]
    a, b = np.take_along_axis(tot32, top, -1), np.take_along_axis(tot64, top, -1)
    ok = np.isfinite(b)
    assert np.isfinite(a[ok]).all() and ok.any()
    report('dense beam scores %s' % (shape,), 'peaked', float(np.abs(logits).max()), G.rel_err(a[ok], b[ok]), 2e-4)


@pytest.mark.parametrize('name', list(R.SCORE_PEAKED_GEOMETRIES))
def test_peaked_projection_operands(name):
    """the operands of tests/test_gpu_score.py::test_score_peaked_logits: W_o scaled, b_o + 200"""
    c = R.score_peaked_case(name)
    cfg, p, out = c['cfg'], c['p'], c['out']
    _, targets, wmask, _ = dr.process_inputs(c['caps'], cfg.token_type)
    want = R.log_softmax_at(out['logits'], targets, wmask)
    live = wmask > 0
    spread = float((out['logits'] - p['b_o'])[live].std())
    assert abs(spread / G.LOGIT_SCALE - 1) < 0.01 and np.abs(out['logits']).max() > 250 and want.min() < -100
    if cfg.softmax_size > 4096:
        assert {R.SCORE_CHUNK - 1, R.SCORE_CHUNK, 0} <= set(targets[live].tolist())
    o32 = dr.train_forward(p, cfg, c['fm'], c['im'], c['caps'], None, None)
    got = R.log_softmax_at(o32['logits'], targets, wmask)
    assert np.isfinite(want).all() and np.isfinite(got).all() and np.isfinite(o32['logits']).all()
    report('token log-probs V=%d' % cfg.softmax_size, 'peaked', spread, S.figure(got, want), F32_RTOL, cap_share=0.1)


# ------------------------------------------------------------------------------------------ whole decoder -----------
@pytest.mark.parametrize('geo', R.FEATURE_GEOMETRIES + R.DECODE_FEATURE_GEOMETRIES,
                         ids=lambda g: 'D%d_M%d_H%d' % (g.get('D', 128), g.get('M', 25), g.get('H', 8)))
def test_features_regime(geo):
    fc = R.features_case(geo)
    cfg, out = fc['cfg'], fc['out']
    assert fc['fm'].min() >= 0 and fc['im'].min() >= 0
    stat = R.z_ratio(out)
    assert abs(stat / R.features_r(geo) - 1) <= 0.2
    g64, dfm64, dim64 = fc['grads'], fc['dfm'], fc['dim']
    o32 = dr.train_forward(fc['p'], cfg, fc['fm'], fc['im'], fc['caps'])
    g32, dfm32, dim32 = dr.train_backward(fc['p'], cfg, o32)
    pairs = dict(logits=(o32['logits'], out['logits']), attn_maps=(o32['attn_maps'], out['attn_maps']),
                 xe=(o32['xe'], out['xe']), dfm=(dfm32, dfm64), dim_embed=(dim32, dim64))
    pairs.update({'grad ' + k: (g32[k], g64[k]) for k in g64})
    worst = 0.0
    for k, (a, b) in pairs.items():
        assert np.isfinite(a).all() and np.isfinite(b).all(), k
        worst = max(worst, G.rel_err(a, b))
    report('train step M=%d H=%d (worst tensor)' % (fc['geo']['M'], fc['geo']['H']), 'features(%d)' % R.features_r(geo), stat,
           worst, F32_RTOL, cap_share=0.1)


# ------------------------------------------------------------------------------------------ shortcuts ---------------
def outside(got, ref, tol):
    return not S.within(got, ref, tol)


def attn_alpha_one_pass(case, inp, dtype=np.float32):
    """dr.attention_scores (add_LN, softmax) with the one-pass LayerNorm, in float32"""
    B, M, D, H = case[:4]
    p = {k: np.asarray(v, dtype) for k, v in inp['p'].items()}
    z = inp['keys'] + inp['q'][:, None, :]
    zhat, _ = G.one_pass_layer_norm(z, p['ln_g'], p['ln_b'])
    raw = (np.tanh(zhat) * p['v']).reshape(B, M, H, D // H).sum(axis=3).transpose(0, 2, 1)
    return dr.softmax(raw / p['tau'], -1)


def test_each_shortcut_lands_outside_the_bar_in_its_regime():
    # 1. no max subtraction, peaked logits
    logits, tg = G.peaked_logits(np.random.default_rng(1), 8, 258, equal_row=0, argmax_row=1, underflow_row=2)
    ref = dr.softmax(R.f64(logits), -1)
    assert not outside(dr.softmax(logits, -1), ref, R.XENT_TOL)
    assert outside(G.softmax_no_max(logits), ref, R.XENT_TOL)
    # 2. loss as -log(softmax[target]), the underflow row
    loss = -np.take_along_axis(dr.log_softmax(R.f64(logits), -1), tg[:, None].astype(np.int64), 1)[:, 0]
    assert not outside(G.loss_from_probability(logits, tg.astype(np.int64), np.float64), loss, R.XENT_TOL)
    assert outside(G.loss_from_probability(logits, tg.astype(np.int64)), loss, R.XENT_TOL)
    # 3. chunk merge without the -inf guard: rows whose first chunk is -inf throughout (a -inf beam, banned tokens)
    x = logits.copy()
    x[3:, :64] = -np.inf
    lse = R.f64(x)[:, -1] - dr.log_softmax(R.f64(x), -1)[:, -1]
    assert not outside(G.lse_merge(x, 64, guard=True), lse, R.XENT_TOL)
    assert outside(G.lse_merge(x, 64, guard=False), lse, R.XENT_TOL)
    # 4. tanh as (e^2x - 1) / (e^2x + 1), saturated attention arguments
    case = ATTN_CASES[0]
    inp = R.attn_inputs(case, regime='saturated')
    ac = R.attn_fwd_ref(case, inp['keys'], inp['values'], inp['q'], inp['p'], None, 1.0)[3]
    arg = (ac['z'] - ac['mean']) * ac['rstd'] * inp['p']['ln_g'] + inp['p']['ln_b']
    assert not outside(np.tanh(arg.astype(np.float32)), np.tanh(arg), R.GATES_TOL)
    assert outside(G.tanh_exp_ratio(arg), np.tanh(arg), R.GATES_TOL)
    # 5. top-p on float32 cumulative sums: the all-equal row of a large vocabulary, p reached deep in the row
    x, _ = G.peaked_logits(np.random.default_rng(2), 4, 25599, equal_row=0)
    keep64, keep32 = G.top_p_keep(x, 0.9), G.top_p_keep(x, 0.9, np.float32)
    assert keep64[0].sum() == math.ceil(0.9 * 25599) and (keep64[1:].sum(1) == 1).all()      # dominant entries: one token
    print('  top-p 0.9 of the uniform row: float64 keeps %d tokens, float32 cumulative sums keep %d' % (keep64[0].sum(), keep32[0].sum()))
    assert (keep64 != keep32).any()
    # 6. one-pass variance at the largest r requested
    inp = R.attn_inputs(case, regime=('offset', 32))
    f64 = R.attn_fwd_ref(case, inp['keys'], inp['values'], inp['q'], inp['p'], None, 1.0)
    z = f64[3]['z']
    _, xh64 = G.two_pass_layer_norm(z, 1.0, 0.0, dtype=np.float64)
    e_two = G.rel_err(G.two_pass_layer_norm(z.astype(np.float32), 1.0, 0.0)[1], xh64)
    e_one = G.rel_err(G.one_pass_layer_norm(z.astype(np.float32), 1.0, 0.0)[1], xh64)
    print('  offset(32) xhat: two-pass float32 %.2e, one-pass float32 %.2e (GATES_TOL %.0e, the bar of a stored xhat)' % (e_two, e_one, R.GATES_TOL))
    assert e_two < R.GATES_TOL < e_one                      # a kernel that stores xhat (LN_LSTM, LN_tanh) cannot pass
    r, e_alpha = 32, G.rel_err(attn_alpha_one_pass(case, inp), f64[0])
    print('  offset(32) alpha through the one-pass form: %.2e (ATTN_FWD_TOL %.0e)' % (e_alpha, R.ATTN_FWD_TOL))
    while e_alpha <= R.ATTN_FWD_TOL and r < 4096:           # not crossed at 32: the crossing r, found by doubling
        r *= 2
        inp_r = R.attn_inputs(case, regime=('offset', r))
        e_alpha = G.rel_err(attn_alpha_one_pass(case, inp_r), R.attn_fwd_ref(case, inp_r['keys'], inp_r['values'], inp_r['q'],
                                                                            inp_r['p'], None, 1.0)[0])
        print('  offset(%d) alpha through the one-pass form: %.2e' % (r, e_alpha))
    assert e_alpha > R.ATTN_FWD_TOL
    assert r == ONE_PASS_ALPHA_CROSSING, r


ONE_PASS_ALPHA_CROSSING = 64       # the attention probabilities leave ATTN_FWD_TOL through a one-pass variance at this r
