"""What the op tests of the executor-only kernel forms (tests/test_gpu_exec_ops.py) rest on, checked without a GPU:
the new C entries are declared, bound and exported consistently; the float64 reference helpers of tests/exec_ops_ref.py
agree with the oracle's own cells, with one step of its train_forward and with the gradient of its forward functions;
and the float32 oracle alone stays inside a quarter of each bar at the shapes the GPU tests use, so three quarters of
every bar are the kernel's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import comic_amd._lib as L
from oracle import decoder_ref as dr
from tests import exec_ops_ref as R
from tests.gpu_util import F32_RTOL, elementwise_excess, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERIES = ('comic_attn_splits', 'comic_attn_bwd_scratch', 'comic_cell_ln_stride', 'comic_gemm_f32_partial')


def _section():
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    decls = {}
    for res, name, args in re.findall(r'\b(int|long|int64_t)\s+(comic_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', header):
        if name.startswith('comic_op_') or name in QUERIES:
            decls[name] = (res, [a.strip() for a in args.split(',')])
    return decls


def test_op_entries_are_declared_bound_and_exported():
    """include/comic_hip.h, _lib._SIGS and the cross-compiled library agree on every op-level entry, argument by argument"""
    decls = _section()
    assert len(decls) == len(QUERIES) + 20, sorted(decls)       # 14 forwarding entries + 6 of the fused / streaming step

    def ctype(a):
        if '*' in a:
            return L.P
        base = a.replace('const', '').split()[0]
        return {'int': C.c_int, 'float': C.c_float, 'int64_t': C.c_int64, 'long': C.c_long}[base]
    for name, (res, args) in decls.items():
        want_res, want_args = L._SIGS[name]
        assert want_res is {'int': C.c_int, 'long': C.c_long, 'int64_t': C.c_int64}[res], name
        assert [ctype(a) for a in args] == list(want_args), name
    defined = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in defined.splitlines() if line.strip())
    assert set(decls) <= exported, set(decls) - exported


def test_internal_prototypes_live_in_one_header():
    """the executors and the op entries read the same list: neither file declares an executor-only form itself"""
    csrc = os.path.join(os.path.dirname(L.LIB_PATH), '..', 'csrc')
    shared = open(os.path.join(csrc, 'exec_entries.h')).read()
    for f in ('decoder_exec.hip', 'op_entries.hip'):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "exec_entries.h"' in text
        for name in re.findall(r'\b(comic_[a-z0-9_]+)\s*\(', shared):
            assert not re.search(r'^(int|long)\s+%s\s*\(' % name, text, flags=re.M), (f, name)


# ---------------------------------------------------------------------------- the helpers against the oracle ---------
def _close(got, ref, tol, name):
    e = rel_err(got, ref)
    assert e <= tol, '%s: %.3e > %.1e' % (name, e, tol)
    return e


def test_cell_references_are_the_oracles_cells():
    """ln_lstm_fwd_ref / ln_lstm_bwd_ref / gru_fwd_ref / gru_bwd_ref start from the finished products; with an identity
    matrix for K the oracle's whole cells compute the same"""
    rng = np.random.default_rng(0)
    B, D = 4, 64
    ln = R.ln_params(rng, D).astype(np.float64)
    g = rng.standard_normal((B, 4 * D))
    c = rng.standard_normal((B, D))
    p = {'K': np.eye(4 * D)}
    for k, n in enumerate(dr.LN_LSTM_NORMS):
        p['cln_%sg' % n], p['cln_%sb' % n] = ln[2 * k], ln[2 * k + 1]
    c2, h2, gates = dr.ln_lstm_cell(p, g, c, np.zeros((B, 0)))
    fw = R.ln_lstm_fwd_ref(g, ln, c)
    _close(fw['c_new'], c2, 1e-12, 'c_new'); _close(fw['h_new'], h2, 1e-12, 'h_new')
    _close(fw['gates_act'], np.concatenate(gates[:4], 1), 1e-12, 'gates')
    _close(fw['xhat'], np.concatenate(gates[5], 1), 1e-12, 'xhat'); _close(fw['rstd'], np.concatenate(gates[6], 1), 1e-12, 'rstd')
    dc2, dh2 = rng.standard_normal((B, D)), rng.standard_normal((B, D))
    cfg = dr.DecoderConfig(rnn_size=D, rnn_name='LN_LSTM')
    grads = {k: np.zeros_like(v) for k, v in p.items()}
    dg_o, dcp_o = dr._cell_backward(p, cfg, grads, gates, g, np.zeros((B, D)), c, dc2, dh2)
    dg, rows, dcp = R.ln_lstm_bwd_ref(fw, ln, c, dc2, dh2)
    _close(dg, dg_o, 1e-11, 'dg'); _close(dcp, dcp_o, 1e-11, 'dc_prev')
    for k, n in enumerate(dr.LN_LSTM_NORMS):
        _close(rows[:, 2 * k].sum(0), grads['cln_%sg' % n], 1e-11, 'gamma ' + n)
        _close(rows[:, 2 * k + 1].sum(0), grads['cln_%sb' % n], 1e-11, 'beta ' + n)
    # GRU, one row at a time (the oracle sums its bias gradients over the batch)
    EA = 2 * D
    A = 0.1 * rng.standard_normal((EA, D))
    Ih = 0.1 * rng.standard_normal((D, D))
    pg = {'K': np.concatenate([np.eye(2 * D), np.zeros((D, 2 * D))]), 'b': 1 + 0.1 * rng.standard_normal(2 * D),
          'K_c': np.concatenate([A, Ih]), 'b_c': 0.1 * rng.standard_normal(D)}
    cfg = dr.DecoderConfig(rnn_size=D, rnn_name='GRU')
    for b in range(B):
        g1, h = rng.standard_normal((1, 2 * D)), rng.standard_normal((1, D))
        _, hn_o, (r_o, u_o, cand_o) = dr.gru_cell(pg, g1, None, h)
        r, u, cand, hn = R.gru_fwd_ref(g1, pg['b'], lambda rh: g1 @ A + rh @ Ih, pg['b_c'], h)
        for name, x, y in (('r', r, r_o), ('u', u, u_o), ('cand', cand, cand_o), ('h_new', hn, hn_o)):
            _close(x, y, 1e-12, name)
        dh2 = rng.standard_normal((1, D))
        grads = {k: np.zeros_like(v) for k, v in pg.items()}
        dxh, _ = dr._cell_backward(pg, cfg, grads, (r, u, cand), np.concatenate([g1, h], 1), h, None, None, dh2)
        drh = (grads['b_c'][None] @ pg['K_c'].T)[:, EA:]
        dpc, dpu, dpr, dh_u, dh_r = R.gru_bwd_ref(r, u, cand, h, dh2, drh)
        _close(dpc, grads['b_c'][None], 1e-11, 'd cand_pre')
        _close(np.concatenate([dpr, dpu], 1), grads['b'][None], 1e-11, 'd gates_pre')
        _close(dh_u + dh_r, dxh[:, EA:], 1e-11, 'd h_prev shares')


def _train_state():
    cfg = dr.DecoderConfig(rnn_size=64, rnn_word_size=32, attn_num_heads=2, softmax_size=50, fm_channels=48, im_embed_size=40,
                           start_id=48, end_id=49, rnn_map_loss_scale=0.7)
    B, M = 4, 9
    rng = np.random.default_rng(5)
    p = dr.init_params(cfg, 1)
    fm = rng.standard_normal((B, M, cfg.fm_channels)).astype(np.float32)
    im = rng.standard_normal((B, cfg.im_embed_size)).astype(np.float32)
    caps = np.full((B, 7), -1, np.int64)
    for b, n in enumerate((5, 2, 4, 3)):
        caps[b, 0] = cfg.start_id
        caps[b, 1:n] = rng.integers(0, 48, n - 1)
        caps[b, n] = cfg.end_id
    masks = dr.make_dropout_masks(cfg, B, 5, M, seed=2)
    return cfg, p, masks, dr.train_forward(p, cfg, fm, im, caps, masks)


def test_helpers_agree_with_one_step_of_train_forward():
    """the epilogue select + input dropout and the map loss, against the state the float32 oracle saved"""
    cfg, p, masks, out = _train_state()
    cc = out['cache']
    E, lens, steps = cfg.rnn_word_size, cc['lens'], cc['steps']
    assert cc['Tp'] == 5 and len(set(lens)) > 2
    keep_in = 1 - cfg.dropout_rnn_in
    for t in range(cc['Tp'] - 1):
        st, nx = steps[t], steps[t + 1]
        assert (t >= lens).any() or t < lens.min()
        att_next, xh = R.epilogue_ref(st['ctx'].astype(np.float64), st['att_prev'].astype(np.float64), lens, t,
                                      masks['inp'][t + 1][:, E:].astype(np.float64), keep_in)
        _close(nx['att_prev'], att_next, R.ATTN_FWD_TOL / 4, 'att_next at t=%d' % t)
        _close(nx['u'][:, E:], xh, R.ATTN_FWD_TOL / 4, 'xh_next at t=%d' % t)
    assert any((t >= lens).any() for t in range(cc['Tp'] - 1))
    hist = np.stack([st['alpha_d'] for st in steps])                              # [Tp,B,H,M]
    loss, dmap = R.map_loss_ref(hist, cfg.rnn_map_loss_scale)
    _close(np.float64(out['map_loss']), loss, R.XENT_TOL / 4, 'map_loss')
    dflat = 2.0 * (cc['flat'] - 1.0) / cc['flat'].size * cfg.rnn_map_loss_scale      # train_backward's d alpha_d, [B,Tp,M]
    _close(dflat.transpose(1, 0, 2), dmap, R.XENT_TOL / 4, 'dmap')


def test_finished_row_rule_is_the_gradient_of_the_oracles_step():
    """attn_bwd_ref with lens: d q and d keys are the derivatives of sum(att_next * G) + sum(sum_h alpha_d * W) through
    the oracle's forward functions and the impute_finished select (central differences in float64)"""
    case = (3, 5, 64, 2, 64, 'add_LN', 'softmax', True)
    B, M, D, H, Cv = case[:5]
    inp = R.attn_inputs(case)
    rng = inp['rng']
    keys, q = inp['keys'].astype(np.float64), inp['q'].astype(np.float64)
    mask = (rng.random((B, H, M)) < 0.9).astype(np.float64)
    lens, t = np.array([3, 1, 5]), 2
    G, Wm, att_prev = rng.standard_normal((B, Cv)), rng.standard_normal((B, M)), rng.standard_normal((B, Cv))

    def loss(keys, q):
        _, alpha_d, ctx, _ = R.attn_fwd_ref(case, keys, keys, q, inp['p'], mask, 0.9)
        return (R.epilogue_ref(ctx, att_prev, lens, t, None, 1.0)[0] * G).sum() + (alpha_d.sum(1) * Wm).sum()
    ref = R.attn_bwd_ref(case, keys, keys, q, inp['p'], mask, 0.9, G, Wm, lens, t)
    eps = 1e-6
    num = np.zeros_like(q)
    for i in np.ndindex(*q.shape):
        d = np.zeros_like(q); d[i] = eps
        num[i] = (loss(keys, q + d) - loss(keys, q - d)) / (2 * eps)
    _close(ref['dq'], num, 1e-6, 'dq')
    dk = ref['dkeys'] + ref['dvalues']
    for i in [(0, 0, 0), (1, 2, 33), (1, 4, 63), (2, 3, 17), (0, 4, 40)]:       # row 1 is finished
        d = np.zeros_like(keys); d[i] = eps
        n = (loss(keys + d, q) - loss(keys - d, q)) / (2 * eps)
        assert abs(dk[i] - n) <= 1e-6 * np.abs(dk).max(), (i, dk[i], n)
    assert np.abs(ref['dvalues'][1]).max() == 0 and np.abs(ref['dkeys'][1]).max() > 0   # no d ctx, but dmap still flows


# ---------------------------------------------------------------------------- the float32 oracle's share of the bars -
FWD_SHAPES = ([c for c, _ in R.SPLIT_CASES] + R.PREFETCH_CASES + [R.HOLE_CASE, R.EPILOGUE_CASES[0]]
              + [(9, 9, 64, 2, 64, 'dot', 'softmax', True), (9, 25, 512, 8, 2048, 'add_LN', 'softmax', False)])


@pytest.mark.parametrize('case', FWD_SHAPES, ids=lambda c: 'x'.join(map(str, c[:5])))
def test_float32_oracle_uses_a_quarter_of_the_forward_bar(case):
    B, M, D, H, Cv = case[:5]
    W = 3 if B == 9 else 1
    inp = R.attn_inputs(case, mem_rows=B // W if W > 1 else None)
    mask = (inp['rng'].random((B, H, M)) < 0.9).astype(np.float32)
    keys, values = R.mem_repeat(inp['keys'], W), R.mem_repeat(inp['values'], W)
    ref = R.attn_fwd_ref(case, keys, values, inp['q'], inp['p'], mask, 0.9)
    f32 = R.attn_fwd_ref(case, keys, values, inp['q'], inp['p'], mask, 0.9, np.float32)
    for name, a, b in zip(('alpha', 'alpha_d', 'ctx'), f32, ref):
        assert a.dtype == np.float32
        _close(a, b, R.ATTN_FWD_TOL / 4, name)


@pytest.mark.parametrize('case', [c for c, _ in R.BWD_CASES], ids=lambda c: 'x'.join(map(str, c[:5])))
def test_float32_oracle_uses_a_quarter_of_the_backward_bar(case):
    B, M, D, H, Cv, method, prob, tied = case
    inp = R.attn_inputs(case)
    mask = (inp['rng'].random((B, H, M)) < 0.9).astype(np.float32)
    rng = np.random.default_rng(B + M + D)
    dctx = rng.standard_normal((B, Cv)).astype(np.float32)
    dmap = (0.01 * rng.standard_normal((B, M))).astype(np.float32)
    lens = np.array([3, 1, 5, 2, 9, 2, 4] * ((B + 6) // 7), np.int32)[:B]
    args = (case, inp['keys'], inp['values'], inp['q'], inp['p'], mask, 0.9, dctx, dmap, lens, 2)
    ref, f32 = R.attn_bwd_ref(*args), R.attn_bwd_ref(*args, dtype=np.float32)
    for k in ('dq', 'dkeys', 'dvalues') + (('pgrad',) if method == 'add_LN' else ()):
        cols = ((0, D), (D, 2 * D), (2 * D, 3 * D), (3 * D, 3 * D + 1)) if k == 'pgrad' else ((0, None),)
        for lo, hi in cols:
            a, b = f32[k][..., lo:hi], ref[k][..., lo:hi]
            _close(a, b, F32_RTOL / 4, '%s[%s:%s]' % (k, lo, hi))
            x = elementwise_excess(a, b, F32_RTOL)
            assert x <= 0.25, '%s[%s:%s]: element-wise share %.2f of the bar' % (k, lo, hi, x)


@pytest.mark.parametrize('D', R.LN_LSTM_D)
def test_float32_oracle_uses_a_quarter_of_the_cell_bars(D):
    rng = np.random.default_rng(D + 3)
    B = 5
    g = (rng.standard_normal((3, B, 4 * D)) / np.sqrt(3)).astype(np.float32)
    ln = R.ln_params(rng, D)
    c = rng.standard_normal((B, D)).astype(np.float32)
    ref = R.ln_lstm_fwd_ref(R.f64(g).sum(0), ln, c)
    f32 = R.ln_lstm_fwd_ref((g[0] + g[1]) + g[2], ln, c, np.float32)
    for k in ref:
        _close(f32[k], ref[k], R.GATES_TOL / 4, k)
    dc2, dh2 = rng.standard_normal((B, D)).astype(np.float32), rng.standard_normal((B, D)).astype(np.float32)
    saved = {k: v.astype(np.float32) for k, v in ref.items()}
    r64 = R.ln_lstm_bwd_ref({k: R.f64(v) for k, v in saved.items()}, ln, c, R.f64(dc2), R.f64(dh2))
    r32 = R.ln_lstm_bwd_ref(saved, ln, c, dc2, dh2, np.float32)
    for name, a, b in zip(('dg', 'rows', 'dc_prev'), r32, r64):
        _close(a, b, F32_RTOL / 4, name)
        assert elementwise_excess(a, b, F32_RTOL) <= 0.25, name
