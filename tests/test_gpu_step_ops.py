"""Op-level parity of the fused and streaming LSTM step kernels (csrc/decoder_fused.hip, csrc/lstm_stream.hip,
csrc/lstm_prep.h, infer_prep_kernel) and of the operand hand-off fused behind the beam merge (csrc/beam_logits.hip), each on
its own operands against float64 numpy (tests/step_ops_ref.py).  Outputs are NaN before the launch, buffers a kernel
accumulates into hold known values, scratch and fragment buffers hold 0xFF bytes (NaN as float32 and as bf16), so an
element left out or a read of an unwritten pad shows.  Each figure is printed before it is asserted (pytest -s).
tests/test_step_ops_ref_cpu.py shows that every deliberate mistake of the references fails these criteria."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import comic_amd._lib as L
from tests import step_ops_ref as S
from tests.gpu_util import DEV, assert_close, dev, lib, stream, sync

NAN = float('nan')
T = S.T_STEP


def nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def ff(nbytes):
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def ptr(t, col=0):
    return None if t is None else t.data_ptr() + 4 * col


def chk(name, got, ref, tol):
    got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = np.asarray(ref, np.float64)
    fin = np.isfinite(got).all()
    print('  %-52s err %.3e  element-wise %.3e  bar %.1e' % (name, S.rel_err(got, ref) if fin else NAN,
                                                              S.elementwise_excess(got, ref, 1.0) if fin else NAN, tol))
    return assert_close(got, ref, tol, name, elementwise=True)


def all_nan(t):
    return bool(torch.isnan(t).all().item())


def all_ff(t):
    return bool((t == 0xFF).all().item())


def cdiv(a, b):
    return (a + b - 1) // b


# ============================================================================ lstm_step_fused ========================
@functools.lru_cache(maxsize=None)
def step_case(shape, regime=None):
    B, D, EA = shape
    inp = S.step_inputs(B, D, EA, regime=regime)
    full = S.lstm_step_ref(inp['xh'], inp['K'], inp['b'], inp['c'], inp['h'], inp['mask'], S.KEEP, inp['lens'], T)
    infer = S.lstm_step_ref(inp['xh'], inp['K'], inp['b'], inp['c'], None, None, 1.0, None, 0)
    return inp, full, infer


def launch_step(shape, full, stop_value=None, regime=None):
    B, D, EA = shape
    Wd = EA + D
    inp = step_case(shape, regime)[0]
    ld_xh, xh_ld, xh_off = Wd + 12, D + 24, 8
    xh = nan(B, ld_xh)
    xh[:, :Wd] = dev(inp['xh'])
    n_panel = cdiv(D, 4) * cdiv(Wd, 16) * 256
    panel = ff(4 * n_panel)
    keep = dict(K=dev(inp['K']), b=dev(inp['b']), c=dev(inp['c']), h=dev(inp['h']), mask=dev(inp['mask']), lens=dev(inp['lens']),
                xh=xh, panel=panel, stop=None if stop_value is None else dev(np.array([stop_value], np.int32)))
    out = dict(gates_act=nan(B, 4 * D), c_new=nan(B, D), y=nan(B, D), c_state=nan(B, D), h_state=nan(B, D), xh_next=nan(B, xh_ld))
    rc = lib().comic_op_lstm_step_fused(
        ptr(keep['K']), ptr(panel), n_panel, ptr(xh), ld_xh, ptr(keep['b']), ptr(keep['c']), ptr(keep['h']) if full else None,
        ptr(out['gates_act']) if full else None, ptr(out['c_new']) if full else None, ptr(out['y']),
        ptr(keep['mask']) if full else None, S.KEEP if full else 1.0, ptr(keep['lens']) if full else None, T if full else 0,
        ptr(out['c_state']), ptr(out['h_state']), ptr(out['xh_next'], xh_off) if full else None, xh_ld, B, D, Wd,
        ptr(keep['stop']), T, stream())
    sync()
    return rc, out, (xh_off, D)


@pytest.mark.parametrize('full', [True, False], ids=['all_outputs', 'inference_call'])
@pytest.mark.parametrize('shape', S.FUSED_SHAPES, ids=str)
def test_lstm_step_fused(shape, full):
    run_lstm_step_fused(shape, full)


@pytest.mark.parametrize('shape', S.FUSED_SHAPES[:2], ids=str)
def test_lstm_step_fused_saturated(shape):
    """the regime `saturated` of tests/regimes.py: gate pre-activations uniform over +-100 (expf(-x) is inf beyond
    88.7), previous cell states to +-50 (tanh(c) = +-1), on the two smallest shapes"""
    run_lstm_step_fused(shape, True, 'saturated')


def run_lstm_step_fused(shape, full, regime=None):
    """lstm_step_fused_wide_kernel<2> over the forward panel of pack_lstm_panels_kernel (mode 0): one unit tile in a
    two-tile workgroup (D = 4), an odd tile count and Wd % 16 = 4 (D = 36, Wd = 68), ragged row tiles, a finished row in
    the last one; operand and xh_next rows wider than Wd / D.  `inference_call`: every optional argument null."""
    B, D, EA = shape
    assert lib() is not None
    _, ref_full, ref_infer = step_case(shape, regime)
    ref = ref_full if full else ref_infer
    rc, out, (off, _) = launch_step(shape, full, regime=regime)
    assert rc == 0, lib().comic_last_error()
    tag = '%s %s: ' % (shape, 'full' if full else 'infer')
    for k in ('y', 'c_state', 'h_state') + (('gates_act', 'c_new') if full else ()):
        chk(tag + k, out[k], ref[k], S.GATES_TOL)
    xn = host(out['xh_next'])
    if full:
        chk(tag + 'xh_next', xn[:, off:off + D], ref['h_state'], S.GATES_TOL)
        assert np.isnan(xn[:, :off]).all() and np.isnan(xn[:, off + D:]).all()
    else:
        assert np.isnan(xn).all() and all_nan(out['gates_act']) and all_nan(out['c_new'])


def test_lstm_step_fused_stop_word():
    """the decode loops' stop word: *stop <= t -> the launch writes nothing; *stop > t -> the step runs"""
    shape = S.FUSED_SHAPES[1]
    rc, out, _ = launch_step(shape, True, stop_value=T)
    assert rc == 0
    assert all(all_nan(v) for v in out.values())
    rc, out, _ = launch_step(shape, True, stop_value=T + 1)
    assert rc == 0
    chk('not stopped: c_state', out['c_state'], step_case(shape)[1]['c_state'], S.GATES_TOL)


def test_lstm_step_fused_refuses_unsupported_shapes():
    """comic_fused_step_supported: D % 4 == 0 && Wd % 4 == 0; anything else is an error, nothing written"""
    B, D, Wd = 3, 6, 16
    out = nan(B, D)
    buf = nan(B * Wd + 4 * D * Wd)
    panel = ff(4 * 4096)
    rc = lib().comic_op_lstm_step_fused(ptr(buf), ptr(panel), 4096, ptr(buf), Wd, None, None, None, None, None, ptr(out), None, 1.0,
                                        None, 0, ptr(out), ptr(out), None, 0, B, D, Wd, None, 0, stream())
    sync()
    assert rc != 0 and all_nan(out) and all_ff(panel)


# ============================================================================ input_grad_fused =======================
@pytest.mark.parametrize('shape', S.GRAD_SHAPES, ids=str)
def test_input_grad_fused(shape):
    run_input_grad_fused(shape)


@pytest.mark.parametrize('shape', S.GRAD_SHAPES[:2], ids=str)
def test_input_grad_fused_saturated(shape):
    """the gate gradients of saturated cells: exact zeros but for one element in eight"""
    run_input_grad_fused(shape, 'saturated')


def run_input_grad_fused(shape, regime=None):
    """input_grad_fused_wide_kernel<2> over the backward panel (mode 1): E | A and A | D inside a 16-feature tile, a
    ragged last feature tile, an odd tile count; carry 0 / 1, mask present / null, demb null"""
    B, E, A, D = shape
    Wd = E + A + D
    inp = S.grad_inputs(B, E, A, D, regime=regime)
    n_panel = cdiv(Wd, 16) * (4 * D // 16) * 256
    d_K, d_dg, d_mask, d_lens = dev(inp['K']), dev(inp['dg']), dev(inp['mask']), dev(inp['lens'])
    for carry, use_mask, use_demb in ((0, True, True), (1, True, True), (1, False, True), (0, False, False)):
        ref = S.input_grad_ref(inp['dg'], inp['K'], inp['mask'] if use_mask else None, S.KEEP, inp['datt'], inp['dh'],
                               inp['lens'], T, carry, E, A)
        panel = ff(4 * n_panel)
        demb, datt, dh = nan(B, E), dev(inp['datt']), dev(inp['dh'])
        rc = lib().comic_op_input_grad_fused(ptr(d_K), ptr(panel), n_panel, ptr(d_dg), ptr(d_mask) if use_mask else None, S.KEEP,
                                             ptr(demb) if use_demb else None, ptr(datt), ptr(dh), ptr(d_lens), T, carry, B, E, A,
                                             D, stream())
        sync()
        assert rc == 0, lib().comic_last_error()
        tag = '%s carry %d mask %d: ' % (shape, carry, use_mask)
        if use_demb:
            chk(tag + 'demb', demb, ref['demb'], S.GATES_TOL)
        else:
            assert all_nan(demb)
        chk(tag + 'datt', datt, ref['datt'], S.GATES_TOL)
        chk(tag + 'dh', dh, ref['dh'], S.GATES_TOL)


# ============================================================================ lstm_grad_fused ========================
@pytest.mark.parametrize('bare', [False, True], ids=['dy_mask_cprev', 'none_of_them'])
@pytest.mark.parametrize('shape', S.QGRAD_SHAPES, ids=str)
def test_lstm_grad_fused(shape, bare):
    run_lstm_grad_fused(shape, bare)


@pytest.mark.parametrize('shape', S.QGRAD_SHAPES[:2], ids=str)
def test_lstm_grad_fused_saturated(shape):
    """the saved activations of a saturated step: s (1 - s) and 1 - tanh^2 underflow, d gates is mostly exact zeros;
    finite everywhere and equal to the reference element-wise, so neither a NaN nor a stray non-zero can hide"""
    run_lstm_grad_fused(shape, False, 'saturated')


def run_lstm_grad_fused(shape, bare, regime=None):
    """lstm_grad_fused_kernel over the W_q panel: dy_total = dy + dq W_q^T, output-dropout and cell backward, the
    finished-row rule; with and without dy / mask_out / c_prev"""
    B, D = shape
    q = S.qgrad_inputs(B, D, regime=regime)
    ref = S.lstm_grad_ref(q['dq'], q['Wq'], q['gates_act'], None if bare else q['c'], q['c_new'], None if bare else q['dy'],
                          None if bare else q['mask'], S.KEEP, q['lens'], T, q['dc'], q['dh'])
    panel = ff(4 * D * D)
    t = {k: dev(q[k]) for k in ('Wq', 'dq', 'gates_act', 'c', 'c_new', 'dy', 'mask', 'lens')}
    dc, dh, dg = dev(q['dc']), dev(q['dh']), nan(B, 4 * D)
    rc = lib().comic_op_lstm_grad_fused(ptr(t['Wq']), ptr(panel), D * D, ptr(t['dq']), ptr(t['gates_act']),
                                        None if bare else ptr(t['c']), ptr(t['c_new']), None if bare else ptr(t['dy']),
                                        None if bare else ptr(t['mask']), S.KEEP, ptr(t['lens']), T, ptr(dc), ptr(dh), ptr(dg), B, D,
                                        stream())
    sync()
    assert rc == 0, lib().comic_last_error()
    tag = '%s %s: ' % (shape, 'bare' if bare else 'full')
    chk(tag + 'dg', dg, ref['dg'], S.GATES_TOL)
    chk(tag + 'dc_state', dc, ref['dc'], S.GATES_TOL)
    fin = T >= q['lens']
    got_dh = host(dh)
    assert (got_dh[~fin] == 0).all() and (got_dh[fin] == q['dh'][fin]).all()


def test_lstm_grad_fused_refuses_d_36():
    """D % 16 != 0: an error (the executor falls back to the unfused chain), nothing written"""
    B, D = 5, 36
    rng = np.random.default_rng(0)
    x = dev(rng.standard_normal((B, 4 * D)).astype(np.float32))
    wq = dev(rng.standard_normal((D, D)).astype(np.float32))
    pre = rng.standard_normal((B, D)).astype(np.float32)
    dc, dh, dg, panel = dev(pre), dev(pre), nan(B, 4 * D), ff(4 * D * D)
    rc = lib().comic_op_lstm_grad_fused(ptr(wq), ptr(panel), D * D, ptr(x), ptr(x), None, ptr(x), None, None, 1.0, None, 0, ptr(dc),
                                        ptr(dh), ptr(dg), B, D, stream())
    sync()
    assert rc != 0
    assert all_nan(dg) and all_ff(panel) and (host(dc) == pre).all() and (host(dh) == pre).all()


# ============================================================================ infer_lstm_step ========================
def xfrag_bytes(R, Kin):
    return cdiv(R, 16) * 16 * cdiv(Kin, 32) * 32 * 4


@functools.lru_cache(maxsize=None)
def infer_case(shape, seed=None, regime=None):
    R, W, D, E, A = shape
    inp = S.infer_inputs(R, W, D, E, A, seed=seed, regime=regime)
    return (inp,) + S.infer_step_ref(inp, W)


def launch_infer(shape, mode, inp=None, stop_value=None, bufs=None):
    """-> rc, outputs; bufs: workspace and fragment buffers of an earlier call over the same shape"""
    R, W, D, E, A = shape
    Wd = E + A + D
    inp = infer_case(shape)[0] if inp is None else inp
    if bufs is None:
        nb = max(int(lib().comic_op_infer_lstm_step_workspace(R, D, E, A, mode)), 256)
        bufs = dict(ws=ff(nb), nb=nb, xf=ff(xfrag_bytes(R, Wd)), yf=ff(xfrag_bytes(R, D)))
    t = {k: dev(inp[k]) for k in ('table', 'ids', 'att', 'h', 'c', 'K', 'b')}
    t['parent'] = None if inp['parent'] is None else dev(inp['parent'])
    t['stop'] = None if stop_value is None else dev(np.array([stop_value], np.int32))
    out = dict(c_in=nan(R, D), c2=nan(R, D), h2=nan(R, D), y=nan(R, D), keep=t, **bufs)
    rc = lib().comic_op_infer_lstm_step(ptr(t['table']), ptr(t['ids']), ptr(t['parent']), W, ptr(t['att']), ptr(t['h']), ptr(t['c']),
                                        ptr(t['K']), ptr(t['b']), ptr(out['c_in']), ptr(out['c2']), ptr(out['h2']), ptr(out['y']),
                                        ptr(out['xf']), ptr(out['yf']), R, E, A, D, inp['V'], mode, ptr(t['stop']), T,
                                        ptr(out['ws']), out['nb'], stream())
    return rc, out


def frag_bits(buf, R, Kin):
    """device fragment buffer -> bf16 bit patterns hi, lo of the live rows [R, 32 ceil(Kin / 32)] (K pads included)"""
    shp = S.frag_shape(R, Kin)
    raw = host(buf)[:int(np.prod(shp)) * 2].view(np.uint16).reshape(shp)
    hi, lo = S.frag_rows(raw)
    return hi[:R], lo[:R]


def check_frag(name, buf, x, R):
    want = S.frag_rows(S.frag_encode(np.ascontiguousarray(x, np.float32)))
    got = frag_bits(buf, R, x.shape[1])
    for part, g, w in zip(('hi', 'lo'), got, want):
        bad = int((g != w[:R]).sum())
        print('  %-52s %d of %d bf16 words differ' % ('%s %s' % (name, part), bad, g.size))
        assert bad == 0, (name, part, np.argwhere(g != w[:R])[:4].tolist())


def check_states(tag, out, ref, tol):
    chk(tag + 'c2', out['c2'], ref['c_state'], tol)
    chk(tag + 'h2', out['h2'], ref['h_state'], tol)
    chk(tag + 'y', out['y'], ref['y'], tol)


@pytest.mark.parametrize('shape', S.INFER_FUSED_SHAPES, ids=str)
def test_infer_lstm_step_fused_path(shape):
    """infer_prep_kernel (embedding | attention, hidden and cell state through the clamped parents, ids outside [0, V) as
    zeros) + the fused step over the gathered rows"""
    inp, x, c_in, ref = infer_case(shape)
    rc, out = launch_infer(shape, 0)
    sync()
    assert rc == 0, lib().comic_last_error()
    np.testing.assert_array_equal(host(out['c_in']), c_in)
    check_states('%s fused: ' % (shape,), out, ref, S.GATES_TOL)
    assert all_ff(out['xf']) and all_ff(out['yf'])


@pytest.mark.parametrize('shape,slices', S.STREAM_SHAPES, ids=lambda v: str(v))
def test_infer_lstm_step_stream_path(shape, slices):
    """lstm_prep_frag_kernel -> lstm_stream_kernel -> lstm_cell_kernel: the operand rows and y as hi / lo fragments bit for
    bit (live rows, K pads included), the gathered cell state bit for bit, the states at the streaming bar; K-slice counts
    1, 3, 5, 7, 8 run the four-at-a-time and the tail loop of the cell kernel's slice sum.
    The four shapes with D % 32 != 0 (D = 16, 48) showed a defect: lstm_cell_kernel left the K pad of y_frag's last k32-step
    unwritten (columns D ... of every live row kept the 0xFF fill), which the query / vocabulary projection multiplies by
    the packed matrix's zero rows -- NaN for stale bits that read as NaN or Inf.  The kernel now zeroes that pad."""
    R, W, D, E, A = shape
    inp, x, c_in, ref = infer_case(shape)
    rc, out = launch_infer(shape, 1)
    sync()
    assert rc == 0, lib().comic_last_error()
    tag = '%s stream S=%d: ' % (shape, slices)
    np.testing.assert_array_equal(host(out['c_in']), c_in)
    check_frag(tag + 'x_frag', out['xf'], x, R)
    y = host(out['y'])
    assert np.isfinite(y).all()
    check_frag(tag + 'y_frag', out['yf'], y, R)
    check_states(tag, out, ref, S.STREAM_TOL)


def test_infer_lstm_step_saturated():
    """comic_op_infer_lstm_step with gate pre-activations over +-100 and cell states to +-50: the fused path on its
    smallest shape, the streaming path on its smallest shape, and both on the shape both serve"""
    for shape, mode, tol in ((S.INFER_FUSED_SHAPES[0], 0, S.GATES_TOL), (S.STREAM_SHAPES[0][0], 1, S.STREAM_TOL),
                             (S.BOTH_SHAPE, 0, S.GATES_TOL), (S.BOTH_SHAPE, 1, S.STREAM_TOL)):
        inp, x, c_in, ref = infer_case(shape, None, 'saturated')
        rc, out = launch_infer(shape, mode, inp=inp)
        sync()
        assert rc == 0, lib().comic_last_error()
        np.testing.assert_array_equal(host(out['c_in']), c_in)
        check_states('%s saturated %s: ' % (shape, 'stream' if mode else 'fused'), out, ref, tol)


def test_infer_lstm_step_stream_and_fused_agree():
    run_stream_and_fused_agree()


def test_infer_lstm_step_stream_and_fused_agree_saturated():
    run_stream_and_fused_agree('saturated')


def run_stream_and_fused_agree(regime=None):
    shape = S.BOTH_SHAPE
    inp = infer_case(shape, None, regime)[0]
    rc1, o1 = launch_infer(shape, 1, inp=inp)
    rc0, o0 = launch_infer(shape, 0, inp=inp)
    sync()
    assert rc1 == 0 and rc0 == 0, lib().comic_last_error()
    np.testing.assert_array_equal(host(o1['c_in']), host(o0['c_in']))
    for k in ('c2', 'h2', 'y'):
        chk('stream vs fused %s' % k, o1[k], host(o0[k]), S.STREAM_TOL)


@pytest.mark.parametrize('R', [32, 257])
def test_infer_lstm_step_stream_refuses_rows_outside_33_256(R):
    shape = (R, 1, 16, 8, 8)
    inp = S.infer_inputs(*shape)
    rc, out = launch_infer(shape, 1, inp=inp)
    sync()
    assert rc != 0
    assert all(all_nan(out[k]) for k in ('c_in', 'c2', 'h2', 'y')) and all_ff(out['xf']) and all_ff(out['yf'])


def test_infer_lstm_step_stop_word():
    for mode, shape in ((1, S.STREAM_SHAPES[1][0]), (0, S.INFER_FUSED_SHAPES[1])):
        rc, out = launch_infer(shape, mode, stop_value=T)
        sync()
        assert rc == 0, lib().comic_last_error()
        assert all(all_nan(out[k]) for k in ('c_in', 'c2', 'h2', 'y')) and all_ff(out['xf']) and all_ff(out['yf'])
        rc, out = launch_infer(shape, mode, stop_value=T + 1)
        sync()
        assert rc == 0
        check_states('not stopped, mode %d: ' % mode, out, infer_case(shape)[3], S.STREAM_TOL if mode else S.GATES_TOL)


def test_infer_lstm_step_stream_back_to_back_calls():
    """three calls over ONE workspace and one pair of fragment buffers, different operands each, no host wait between
    them: each equals its own reference (a K-slice or a fragment left from the call before would show)"""
    shape = S.STREAM_SHAPES[2][0]
    R, W, D, E, A = shape
    cases = [infer_case(shape, seed) for seed in (11, 12, 13)]
    outs, bufs = [], None
    for inp, _, _, _ in cases:
        rc, out = launch_infer(shape, 1, inp=inp, bufs=bufs)
        assert rc == 0, lib().comic_last_error()
        bufs = {k: out[k] for k in ('ws', 'nb', 'xf', 'yf')}
        outs.append(out)
    sync()
    for i, ((inp, x, c_in, ref), out) in enumerate(zip(cases, outs)):
        np.testing.assert_array_equal(host(out['c_in']), c_in)
        check_states('call %d: ' % i, out, ref, S.STREAM_TOL)
    check_frag('last call x_frag', bufs['xf'], cases[-1][1], R)


# ============================================================================ beam_step_prep =========================
@pytest.mark.parametrize('shape', S.PREP_SHAPES, ids=str)
def test_beam_step_prep(shape):
    """The beam step that also prepares the NEXT step's operand rows (merge kernel at V >= 4096, small step at V <= 1024):
    its own outputs equal comic_beam_step_dense's bit for bit, and the rows / cell state it leaves are the gather through
    the words and parents the device chose (one finished beam, one all-finished entry)."""
    B, W, V, D, E, A = shape
    R, Wd, end = B * W, E + A + D, V - 1
    assert Wd % 32 != 0
    rng = np.random.default_rng(B + W + V)
    y = rng.standard_normal((R, D)).astype(np.float32)
    Wo = (rng.standard_normal((D, V)) / np.sqrt(D)).astype(np.float32)
    bo = (0.1 * rng.standard_normal(V)).astype(np.float32)
    lp = np.tile(np.linspace(0, -2.0, W, dtype=np.float32), (B, 1))
    fin = np.zeros((B, W), np.int32); fin[0, 1] = 1; fin[B - 1] = 1
    lens = rng.integers(0, 5, (B, W)).astype(np.int64)
    table = rng.standard_normal((V, E)).astype(np.float32)
    att, h, c = (rng.standard_normal((R, n)).astype(np.float32) for n in (A, D, D))
    d = {k: dev(v) for k, v in dict(y=y, Wo=Wo, bo=bo, table=table, att=att, h=h, c=c).items()}
    nb = int(lib().comic_beam_step_dense_workspace(B, W, D, V))
    res = []
    for prep in (False, True):
        st = dict(lp=dev(lp), fin=dev(fin), lens=dev(lens), word=torch.full((B, W), -7, dtype=torch.int32, device=DEV),
                  par=torch.full((B, W), -7, dtype=torch.int32, device=DEV), sc=nan(B, W), ws=ff(nb), xf=ff(xfrag_bytes(R, Wd)),
                  c_in=nan(R, D))
        common = (ptr(d['y']), ptr(d['Wo']), ptr(d['bo']), ptr(st['lp']), ptr(st['fin']), ptr(st['lens']), ptr(st['word']),
                  ptr(st['par']), ptr(st['sc']), B, W, D, V, end)
        if prep:
            rc = lib().comic_op_beam_step_prep(*common, ptr(d['table']), ptr(d['att']), ptr(d['h']), ptr(d['c']), ptr(st['xf']),
                                               ptr(st['c_in']), E, A, ptr(st['ws']), nb, stream())
        else:
            rc = lib().comic_beam_step_dense(*common, ptr(st['ws']), nb, stream())
        sync()
        assert rc == 0, lib().comic_last_error()
        res.append(st)
    dense, prep = res
    for k in ('word', 'par', 'fin', 'lens'):
        np.testing.assert_array_equal(host(prep[k]), host(dense[k]), err_msg=k)
    for k in ('sc', 'lp'):
        np.testing.assert_array_equal(host(prep[k]).view(np.uint32), host(dense[k]).view(np.uint32), err_msg=k)
    assert all_nan(dense['c_in']) and all_ff(dense['xf'])
    words, parents = host(prep['word']).reshape(R), host(prep['par']).reshape(R)
    assert (parents >= 0).all() and (parents < W).all() and (words >= 0).all() and (words < V).all()
    assert (parents != np.arange(R) % W).any()
    x, c_in = S.gather_ref(table, words, parents, W, att, h, c, V)
    np.testing.assert_array_equal(host(prep['c_in']), c_in)
    check_frag('%s next x_frag' % (shape,), prep['xf'], x, R)


def test_beam_step_prep_refuses_a_shape_no_kernel_serves():
    """V = 2000: neither the merge kernel (V >= 4096) nor the small step (V <= 1024)"""
    B, W, V, D, E, A = 2, 3, 2000, 64, 8, 8
    R = B * W
    z = nan(max(D * V, R * D, V * E))
    st = dict(lp=nan(B, W), fin=torch.zeros((B, W), dtype=torch.int32, device=DEV),
              lens=torch.zeros((B, W), dtype=torch.int64, device=DEV), word=torch.full((B, W), -7, dtype=torch.int32, device=DEV),
              par=torch.full((B, W), -7, dtype=torch.int32, device=DEV), sc=nan(B, W))
    nb = int(lib().comic_beam_step_dense_workspace(B, W, D, V))
    ws, xf, c_in = ff(nb), ff(xfrag_bytes(R, E + A + D)), nan(R, D)
    rc = lib().comic_op_beam_step_prep(ptr(z), ptr(z), ptr(z), ptr(st['lp']), ptr(st['fin']), ptr(st['lens']), ptr(st['word']),
                                       ptr(st['par']), ptr(st['sc']), B, W, D, V, V - 1, ptr(z), ptr(z), ptr(z), ptr(z), ptr(xf),
                                       ptr(c_in), E, A, ptr(ws), nb, stream())
    sync()
    assert rc != 0
    assert all_nan(c_in) and all_ff(xf) and all_nan(st['sc']) and (host(st['word']) == -7).all()
