"""What tests/test_gpu_step_ops.py rests on, checked without a GPU: the float64 references of tests/step_ops_ref.py are
the oracle's BasicLSTMCell forward and backward; the fragment codec round-trips; every deliberate mistake (mutant) of a
reference FAILS the GPU test's own criterion at the GPU test's own shapes and inputs, so the bars and inputs can tell a
kernel with that mistake from a correct one; and the bars come from the reference side: float32 numpy uses under a
quarter of GATES_TOL on the exact-fp32 forms, and the streaming bar is four times the error of a float32 emulation of
the kernel's split arithmetic."""
import numpy as np
import pytest

import comic_amd._lib as L
from oracle import decoder_ref as dr
from tests import step_ops_ref as S
from tests.exec_ops_ref import f64

T = S.T_STEP


def _close(got, ref, tol, name):
    e = S.rel_err(got, ref)
    assert e <= tol, '%s: %.3e > %.1e' % (name, e, tol)


def test_new_entries_are_in_the_binding_table():
    for name in ('comic_op_lstm_step_fused', 'comic_op_input_grad_fused', 'comic_op_lstm_grad_fused',
                 'comic_op_infer_lstm_step_workspace', 'comic_op_infer_lstm_step', 'comic_op_beam_step_prep'):
        assert name in L.EXPORTED_SYMBOLS


# ---------------------------------------------------------------------------- the references against the oracle ------
def test_step_and_backward_references_are_the_oracles_cell():
    rng = np.random.default_rng(1)
    B, E, A, D = 5, 6, 10, 12
    EA = E + A
    inp = {k: f64(v) for k, v in S.step_inputs(B, D, EA).items() if k != 'lens'}
    p = {'K': inp['K'], 'b': inp['b']}
    c2, h2, gates = dr.lstm_cell(p, inp['xh'][:, :EA], inp['c'], inp['xh'][:, EA:])
    ref = S.lstm_step_ref(inp['xh'], inp['K'], inp['b'], inp['c'], inp['h'], None, 1.0, None, 0)
    _close(ref['c_new'], c2, 1e-12, 'c_new'); _close(ref['h_new'], h2, 1e-12, 'h_new')
    _close(ref['gates_act'], np.concatenate(gates[:4], 1), 1e-12, 'gates')
    for k in ('c_state', 'h_state', 'y'):
        _close(ref[k], c2 if k == 'c_state' else h2, 1e-12, k)
    # output dropout and the finished-row select, stated once more in plain numpy
    lens = np.array([3, 1, 5, 2, 9], np.int32)
    full = S.lstm_step_ref(inp['xh'], inp['K'], inp['b'], inp['c'], inp['h'], inp['mask'], S.KEEP, lens, T)
    fin = np.array([False, True, False, True, False])
    _close(full['y'], h2 / S.KEEP * inp['mask'], 1e-12, 'y')
    assert (full['c_state'][fin] == inp['c'][fin]).all() and (full['h_state'][fin] == inp['h'][fin]).all()
    assert (full['c_state'][~fin] == c2[~fin]).all() and (full['h_state'][~fin] == h2[~fin]).all()
    # backward: W_q = 0 leaves dy alone; the oracle's cell backward gives dg, d c_prev and d [x;att;h]
    dc2, dh2 = rng.standard_normal((B, D)), rng.standard_normal((B, D))
    cfg = dr.DecoderConfig(rnn_size=D)
    assert cfg.rnn_name == 'LSTM'
    grads = {k: np.zeros_like(v) for k, v in p.items()}
    dxh_o, dcp_o = dr._cell_backward(p, cfg, grads, gates, inp['xh'], inp['xh'][:, EA:], inp['c'], dc2, dh2)
    bw = S.lstm_grad_ref(np.zeros((B, D)), np.zeros((D, D)), ref['gates_act'], inp['c'], ref['c_new'], dh2, None, 1.0, None, 0,
                         dc2, np.zeros((B, D)))
    _close(bw['dc'], dcp_o, 1e-12, 'd c_prev')
    assert np.abs(bw['dh']).max() == 0
    ig = S.input_grad_ref(bw['dg'], inp['K'], None, 1.0, np.zeros((B, A)), np.zeros((B, D)), None, 0, 0, E, A)
    _close(np.concatenate([ig['demb'], ig['datt'], ig['dh']], 1), dxh_o, 1e-12, 'd [x;att;h]')
    # dy_total = dy + dq W_q^T: the query projection q = y W_q of the step, so d y gets dq W_q^T
    Wq, dq = rng.standard_normal((D, D)), rng.standard_normal((B, D))
    b2 = S.lstm_grad_ref(dq, Wq, ref['gates_act'], inp['c'], ref['c_new'], dh2, None, 1.0, None, 0, dc2, np.zeros((B, D)))
    dg_o, _ = dr._lstm_backward(None, gates, inp['c'], dc2, dh2 + dq @ Wq.T, D)
    _close(b2['dg'], dg_o, 1e-12, 'dg with dq')


def test_carry_and_finished_rules_of_the_backward_references():
    B, E, A, D = 6, 3, 5, 4
    inp = S.grad_inputs(B, E, A, D)
    lens = np.array([3, 1, 5, 2, 9, 2], np.int32)
    fin = T >= lens
    assert fin.any() and not fin.all()
    r0 = S.input_grad_ref(inp['dg'], inp['K'], inp['mask'], S.KEEP, inp['datt'], inp['dh'], lens, T, 0, E, A)
    r1 = S.input_grad_ref(inp['dg'], inp['K'], inp['mask'], S.KEEP, inp['datt'], inp['dh'], lens, T, 1, E, A)
    d = f64(inp['dg']) @ f64(inp['K']).T
    v = d[:, E:E + A] / S.KEEP * inp['mask'][:, E:]
    _close(r0['datt'], inp['datt'] + v, 1e-12, 'datt, no carry')
    _close(r1['datt'][fin], (inp['datt'] + v)[fin], 1e-12, 'datt, carry, finished')
    _close(r1['datt'][~fin], v[~fin], 1e-12, 'datt, carry, live')
    _close(r0['dh'], inp['dh'] + d[:, E + A:], 1e-12, 'dh')
    _close(r0['demb'], d[:, :E] / S.KEEP * inp['mask'][:, :E], 1e-12, 'demb')


def test_gather_reference():
    inp = S.infer_inputs(12, 3, 8, 8, 8)
    x, c_in = S.gather_ref(inp['table'], inp['ids'], inp['parent'], 3, inp['att'], inp['h'], inp['c'], inp['V'])
    for r in range(12):
        src = (r // 3) * 3 + min(max(int(inp['parent'][r]), 0), 2)
        idr = int(inp['ids'][r])
        emb = inp['table'][idr] if 0 <= idr < inp['V'] else np.zeros(8, np.float32)
        assert (x[r] == np.concatenate([emb, inp['att'][src], inp['h'][src]])).all() and (c_in[r] == inp['c'][src]).all()
    assert inp['parent'].min() == -1 and inp['parent'].max() == 6 and inp['ids'].min() == -1 and inp['ids'].max() == inp['V']
    assert (inp['parent'] != np.arange(12) % 3).any()


# ---------------------------------------------------------------------------- fragment codec -------------------------
@pytest.mark.parametrize('R,Kin', [(1, 8), (33, 32), (48, 96), (129, 160), (150, 416), (40, 88)])
def test_fragment_codec_round_trips(R, Kin):
    rng = np.random.default_rng(R + Kin)
    x = (rng.standard_normal((R, Kin)) * np.exp(3 * rng.standard_normal((R, Kin)))).astype(np.float32)
    frag = S.frag_encode(x)
    assert frag.shape == S.frag_shape(R, Kin) and frag.dtype == np.uint16
    hi, lo = S.frag_decode(frag, R, Kin)
    h0, l0 = S.split_hi_lo(x)
    assert (hi == h0).all() and (lo == l0).all()
    assert (np.abs(f64(x) - (f64(hi) + f64(lo))) <= 2.0 ** -16 * np.abs(f64(x))).all()
    # the documented lane: row r, segment sg -> tile r / 16, k-step sg / 4, lane (r % 16) + 16 (sg % 4)
    r, sg = R - 1, Kin // 8 - 1
    want = (h0[r, sg * 8:sg * 8 + 8].view(np.uint32) >> 16).astype(np.uint16)
    assert (frag[r // 16, sg // 4, 0, (r % 16) + 16 * (sg % 4)] == want).all()
    # rows beyond R and features beyond Kin are zero bits
    bh, bl = S.frag_rows(frag)
    assert not bh[R:].any() and not bl[R:].any() and not bh[:, Kin:].any() and not bl[:, Kin:].any()


def test_stream_slice_counts():
    for (R, W, D, E, A), want in S.STREAM_SHAPES:
        assert S.stream_slices(4 * D, E + A + D)[1] == want
    assert S.stream_slices(4 * 512, 2816) == (11, 8)


# ---------------------------------------------------------------------------- sensitivity ----------------------------
def _fails(got, ref, keys, tol):
    return any(not S.within(got[k], ref[k], tol) for k in keys)


STEP_KEYS = ('gates_act', 'c_new', 'y', 'c_state', 'h_state')


@pytest.mark.parametrize('shape', S.FUSED_SHAPES, ids=str)
def test_every_mutant_of_the_step_fails_the_gpu_criterion(shape):
    B, D, EA = shape
    inp = S.step_inputs(B, D, EA)
    args = (inp['xh'], inp['K'], inp['b'], inp['c'], inp['h'], inp['mask'], S.KEEP, inp['lens'], T)
    ref = S.lstm_step_ref(*args)
    fin = T >= inp['lens']
    for mut in S.MUTANTS_STEP:
        if mut == 'fin' and not fin.any():
            continue                                      # one live row: nothing to hold
        assert _fails(S.lstm_step_ref(*args, mut=mut), ref, STEP_KEYS, S.GATES_TOL), (shape, mut)
        if mut not in ('keep', 'fin'):                    # the inference call: y, c_state, h_state alone
            inf = (inp['xh'], inp['K'], inp['b'], inp['c'], None, None, 1.0, None, 0)
            assert _fails(S.lstm_step_ref(*inf, mut=mut), S.lstm_step_ref(*inf), ('y', 'c_state', 'h_state'), S.GATES_TOL), (shape, mut)
    assert fin.any() or B == 1


@pytest.mark.parametrize('shape', S.GRAD_SHAPES, ids=str)
def test_every_mutant_of_the_input_gradient_fails_the_gpu_criterion(shape):
    B, E, A, D = shape
    inp = S.grad_inputs(B, E, A, D)
    for carry in (0, 1):
        args = (inp['dg'], inp['K'], inp['mask'], S.KEEP, inp['datt'], inp['dh'], inp['lens'], T, carry, E, A)
        ref = S.input_grad_ref(*args)
        for mut in S.MUTANTS_INPUT_GRAD:
            if mut == 'carry' and (not carry or (T >= inp['lens']).all()):
                continue
            assert _fails(S.input_grad_ref(*args, mut=mut), ref, ('demb', 'datt', 'dh'), S.GATES_TOL), (shape, carry, mut)


@pytest.mark.parametrize('shape', S.QGRAD_SHAPES, ids=str)
def test_every_mutant_of_the_cell_gradient_fails_the_gpu_criterion(shape):
    B, D = shape
    q = S.qgrad_inputs(B, D)
    args = (q['dq'], q['Wq'], q['gates_act'], q['c'], q['c_new'], q['dy'], q['mask'], S.KEEP, q['lens'], T, q['dc'], q['dh'])
    ref = S.lstm_grad_ref(*args)
    for mut in S.MUTANTS_QGRAD:
        if mut == 'fin' and not (T >= q['lens']).any():
            continue
        assert _fails(S.lstm_grad_ref(*args, mut=mut), ref, ('dg', 'dc', 'dh'), S.GATES_TOL), (shape, mut)


@pytest.mark.parametrize('shape', S.INFER_FUSED_SHAPES + [c for c, _ in S.STREAM_SHAPES[:4]], ids=str)
def test_every_mutant_of_the_decode_step_fails_the_gpu_criterion(shape):
    R, W, D, E, A = shape
    inp = S.infer_inputs(R, W, D, E, A)
    streamed = R > 32
    x, c_in, ref = S.infer_step_ref(inp, W)
    for mut in S.MUTANTS_GATHER:                            # bit-exact criterion on the gathered rows
        if W == 1 and mut != 'bad_id':
            continue                                        # greedy rows: no parents
        xm, cm, _ = S.infer_step_ref(inp, W, gather_mut=mut)
        assert not ((xm == x).all() and (cm == c_in).all()), (shape, mut)
        if streamed:
            assert not (S.frag_encode(xm) == S.frag_encode(x)).all(), (shape, mut)
    tol = S.STREAM_TOL if streamed else S.GATES_TOL
    for mut in (S.MUTANTS_STREAM if streamed else [m for m in S.MUTANTS_STEP if m not in ('keep', 'fin')]):
        if streamed or mut != 'k_tail':
            out = S.infer_step_ref(inp, W, mut=mut)[2]
        else:
            out = S.lstm_step_ref(x, inp['K'], inp['b'], c_in, None, None, 1.0, None, 0, mut=mut)
        assert _fails(out, ref, ('c_state', 'h_state', 'y'), tol), (shape, mut)


# ---------------------------------------------------------------------------- the bars -------------------------------
def _quarter(f32, ref, keys, tag):
    for k in keys:
        assert f32[k].dtype == np.float32, k
        e = S.figure(f32[k], ref[k])
        print('  %-40s float32 numpy %.2e  quarter bar %.1e' % (tag + ' ' + k, e, S.GATES_TOL / 4))
        assert e <= S.GATES_TOL / 4, (tag, k, e)


@pytest.mark.parametrize('shape', S.FUSED_SHAPES, ids=str)
def test_float32_numpy_uses_a_quarter_of_the_step_bar(shape):
    B, D, EA = shape
    inp = S.step_inputs(B, D, EA)
    args = (inp['xh'], inp['K'], inp['b'], inp['c'], inp['h'], inp['mask'], S.KEEP, inp['lens'], T)
    _quarter(S.lstm_step_ref(*args, dtype=np.float32), S.lstm_step_ref(*args), STEP_KEYS, 'step %s' % (shape,))


@pytest.mark.parametrize('shape', S.GRAD_SHAPES, ids=str)
def test_float32_numpy_uses_a_quarter_of_the_input_gradient_bar(shape):
    B, E, A, D = shape
    inp = S.grad_inputs(B, E, A, D)
    args = (inp['dg'], inp['K'], inp['mask'], S.KEEP, inp['datt'], inp['dh'], inp['lens'], T, 1, E, A)
    _quarter(S.input_grad_ref(*args, dtype=np.float32), S.input_grad_ref(*args), ('demb', 'datt', 'dh'), 'input grad %s' % (shape,))


@pytest.mark.parametrize('shape', S.QGRAD_SHAPES, ids=str)
def test_float32_numpy_uses_a_quarter_of_the_cell_gradient_bar(shape):
    q = S.qgrad_inputs(*shape)
    args = (q['dq'], q['Wq'], q['gates_act'], q['c'], q['c_new'], q['dy'], q['mask'], S.KEEP, q['lens'], T, q['dc'], q['dh'])
    _quarter(S.lstm_grad_ref(*args, dtype=np.float32), S.lstm_grad_ref(*args), ('dg', 'dc'), 'cell grad %s' % (shape,))


@pytest.mark.parametrize('shape', S.INFER_FUSED_SHAPES, ids=str)
def test_float32_numpy_uses_a_quarter_of_the_decode_step_bar(shape):
    R, W, D, E, A = shape
    inp = S.infer_inputs(R, W, D, E, A)
    x, c_in, ref = S.infer_step_ref(inp, W)
    f32 = S.lstm_step_ref(x, inp['K'], inp['b'], c_in, None, None, 1.0, None, 0, dtype=np.float32)
    _quarter(f32, ref, ('c_state', 'h_state', 'y'), 'decode step %s' % (shape,))


def test_stream_bar_is_four_times_the_emulation():
    """float32 emulation of hi*hi + hi*lo + lo*hi with the K-slices added in slice order, against float64 on the same
    float32 operands, at every streaming shape: the bar is 4 x the largest figure (and at most 5e-5)"""
    worst = worst_el = 0.0
    for (R, W, D, E, A), _ in S.STREAM_SHAPES:
        inp = S.infer_inputs(R, W, D, E, A)
        ref = S.infer_step_ref(inp, W)[2]
        emu = S.infer_step_ref(inp, W, emulate=True)[2]
        figs = [S.rel_err(emu[k], ref[k]) for k in ('c_state', 'h_state', 'y')]
        els = [S.elementwise_excess(emu[k], ref[k], 1.0) for k in ('c_state', 'h_state', 'y')]
        print('  %-24s emulation c2 %.2e  h2 %.2e  y %.2e   element-wise %.2e  %.2e  %.2e' % ((R, W, D, E, A), *figs, *els))
        worst, worst_el = max(worst, *figs), max(worst_el, *els)
        assert all(S.within(emu[k], ref[k], S.STREAM_TOL) for k in ('c_state', 'h_state', 'y'))
    print('  largest %.2e -> 4 x = %.2e, STREAM_TOL %.1e; element-wise share of the emulation %.0f %%'
          % (worst, 4 * worst, S.STREAM_TOL, 100 * worst_el / S.STREAM_TOL))
    assert 4 * worst <= S.STREAM_TOL <= S.STREAM_TOL_CAP
    assert S.STREAM_TOL <= 4 * worst * 1.02             # ... and no looser than that figure rounded up
