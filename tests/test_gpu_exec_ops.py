"""Op-level parity of the EXECUTOR-ONLY forms of the decoder kernels: the forms training, greedy / beam decode,
sampling and scoring launch (split attention, fused epilogue, shared memories, split backward, fused losses, the
LN_LSTM / GRU cells, split-K partials), each on its own operands against float64 numpy (tests/exec_ops_ref.py).
Every output is NaN before the launch, so an element the kernel leaves out fails the finiteness check; buffers a kernel
accumulates into are prefilled with known values.  Each figure is printed before it is asserted (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import comic_amd._lib as L
from oracle import decoder_ref as dr
from tests import exec_ops_ref as R
from tests import regimes as G
from tests.gpu_util import DEV, F32_RTOL, P, assert_close, dev, elementwise_excess, lib, stream, sync

NAN = float('nan')


def nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def chk(name, got, ref, tol, elementwise=None, restated=None):
    """elementwise=True: the element-wise criterion of gpu_util beside the max-norm one at any bar (the peaked and
    saturated regimes of tests/regimes.py, whose tensors span many magnitudes).  restated: the error of the float32
    restatement of the reference on the same operands; the bar is then regimes.bar(tol, restated), printed beside it."""
    if restated is not None:
        name, tol = '%s [float32 restatement %.2e]' % (name, restated), G.bar(tol, restated)
    got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = np.asarray(ref, np.float64)
    fin = np.isfinite(got).all()
    e = float(np.abs(got.astype(np.float64) - ref).max() / (np.abs(ref).max() + 1e-30)) if fin else NAN
    if elementwise:
        print('  %-44s err %.3e  element-wise %.3e  bar %.1e' % (name, e, elementwise_excess(got, ref, 1.0) if fin else NAN, tol))
    else:
        print('  %-44s err %.3e  bar %.1e' % (name, e, tol))
    return assert_close(got, ref, tol, name, elementwise=elementwise)


# The regimes of tests/regimes.py the attention / LayerNorm kernels run in.  The attention forward and the LN_LSTM forward
# compute the float32 restatement of their reference here, print its error and take their bar from regimes.bar().  Every
# other case below uses its op's normal bar as a constant: that is sound only because tests/test_regimes_cpu.py holds the
# restatement below a quarter of that bar ON THE SAME OPERANDS -- both sides must build them with the same shared builder
# (attn_inputs, ln_lstm_regime, saturate_partials, xent_operands_peaked, step_ops_ref's *_inputs) at the same shapes and
# seeds.  A case added or re-seeded here needs its twin there.
ATTN_REGIMES = [('offset', 4), ('offset', 32), 'saturated']
LN_LSTM_REGIMES = [('offset', 4), ('offset', 8), 'saturated']           # 8, not 32: see tests/test_regimes_cpu.py


def ew(regime):
    """peaked and saturated regimes get the element-wise check too"""
    return True if regime in ('saturated', 'peaked') else None


def ptr(t, col=0):
    return None if t is None else t.data_ptr() + 4 * col


def desc(case, B=None):
    b, M, D, H, Cv, method, prob, tied = case
    return L.AttnDesc(B=b if B is None else B, M=M, D=D, H=H, Cv=Cv, method=0 if method == 'add_LN' else 1,
                      prob=0 if prob == 'softmax' else 1, tied=int(tied))


# ============================================================================ attention, forward =====================
class Fwd:
    """operands of one case on the device + the float64 reference, computed once and left unchanged"""

    def __init__(self, case, use_mask, mem_div=1, regime=None):
        B, M, D, H, Cv, method, prob, tied = case
        self.case, self.keep, self.mem_div, self.regime = case, 0.9, mem_div, regime
        inp = R.attn_inputs(case, mem_rows=B // mem_div if mem_div > 1 else None, regime=regime)
        self.inp = inp
        self.mask = (inp['rng'].random((B, H, M)) < self.keep).astype(np.float32) if use_mask else None
        keys, values = inp['keys'], inp['values']
        if mem_div > 1:
            keys, values = R.mem_repeat(keys, mem_div), R.mem_repeat(values, mem_div)
        self.alpha, self.alpha_d, self.ctx, _ = R.attn_fwd_ref(case, keys, values, inp['q'], inp['p'], self.mask, self.keep)
        self.restated = dict(alpha=None, alpha_d=None, ctx=None)
        if regime is not None:                                  # the float32 oracle on the same operands, for the bar rule
            with np.errstate(over='ignore'):
                r32 = R.attn_fwd_ref(case, keys, values, inp['q'], inp['p'], self.mask, self.keep, dtype=np.float32)
            self.restated = {k: G.rel_err(a, b) for k, a, b in zip(('alpha', 'alpha_d', 'ctx'), r32,
                                                                   (self.alpha, self.alpha_d, self.ctx))}
        self.d_keys = dev(inp['keys'])
        self.d_values = self.d_keys if tied else dev(inp['values'])
        self.d_q = dev(inp['q'])
        self.d_p = {k: dev(v.reshape(-1)) for k, v in inp['p'].items()}
        self.d_mask = dev(self.mask) if use_mask else None


@functools.lru_cache(maxsize=2)
def fwd_case(case, use_mask, mem_div=1, regime=None):
    return Fwd(case, use_mask, mem_div, regime)


def launch_fwd(f, scratch, q=None, q_parts=1, q_out=None, lens=None, t=0, att_prev=None, att_next=None, xh_next=None,
               xh_ld=0, mask_next=None, mask_ld=0, keep_in=1.0, B=None):
    """-> rc, alpha, alpha_d, ctx (NaN-filled before the launch)"""
    b, M, D, H, Cv = f.case[:5]
    B = b if B is None else B
    d = desc(f.case, B)
    alpha, alpha_d, ctx = nan(B, H, M), nan(B, H, M), nan(B, Cv)
    ws = nan(B * H * M) if scratch else None
    rc = lib().comic_op_attn_fwd(C.byref(d), ptr(f.d_keys), ptr(f.d_values), ptr(f.d_q if q is None else q), ptr(f.d_p['ln_g']),
                                 ptr(f.d_p['ln_b']), ptr(f.d_p['v']), ptr(f.d_p['tau']), ptr(f.d_mask), f.keep, ptr(alpha),
                                 ptr(alpha_d), ptr(ctx), ptr(lens), t, ptr(att_prev), ptr(att_next), xh_next, xh_ld,
                                 mask_next, mask_ld, keep_in, q_parts, ptr(q_out), ptr(ws), f.mem_div, stream())
    sync()
    return rc, alpha, alpha_d, ctx


def check_fwd(f, out, tag):
    rc, alpha, alpha_d, ctx = out
    assert rc == 0, (tag, lib().comic_last_error())
    chk(tag + ' alpha', alpha, f.alpha, R.ATTN_FWD_TOL, ew(f.regime), f.restated['alpha'])
    chk(tag + ' alpha_d', alpha_d, f.alpha_d, R.ATTN_FWD_TOL, ew(f.regime), f.restated['alpha_d'])
    chk(tag + ' ctx', ctx, f.ctx, R.ATTN_FWD_TOL, ew(f.regime), f.restated['ctx'])


@pytest.mark.parametrize('regime', ATTN_REGIMES, ids=str)
@pytest.mark.parametrize('case,S', R.SPLIT_CASES[:2], ids=lambda v: 'x'.join(map(str, v[:5])) if isinstance(v, tuple) else 'S%d' % v)
def test_attn_fwd_forms_off_unit_scale(case, S, regime):
    """the one-workgroup and the split form on LayerNorm rows with a mean of 4 and 32 standard deviations and with the
    gains x 40 (tanh arguments to +-180: both branches of fast_tanh, __expf overflow); the two smallest add_LN entries
    of SPLIT_CASES, softmax / tied and sigmoid / independent"""
    assert lib().comic_attn_splits(case[0], case[1]) == S
    f = fwd_case(case, True, 1, regime)
    check_fwd(f, launch_fwd(f, scratch=False), '%s one-workgroup:' % (regime,))
    check_fwd(f, launch_fwd(f, scratch=True), '%s split S=%d:' % (regime, S))


@pytest.mark.parametrize('use_mask', [False, True])
@pytest.mark.parametrize('case,S', R.SPLIT_CASES, ids=lambda v: 'x'.join(map(str, v[:5])) if isinstance(v, tuple) else 'S%d' % v)
def test_attn_fwd_split_form(case, S, use_mask):
    """attn_scores_kernel + attn_ctx_kernel with S workgroups per batch row; the same operands without scratch run the
    one-workgroup form against the same reference: a failure of the split form alone is a bug of the split."""
    assert lib().comic_attn_splits(case[0], case[1]) == S
    f = fwd_case(case, use_mask)
    check_fwd(f, launch_fwd(f, scratch=False), 'one-workgroup:')
    check_fwd(f, launch_fwd(f, scratch=True), 'split S=%d:' % S)


@pytest.mark.parametrize('use_mask', [False, True])
@pytest.mark.parametrize('case', R.PREFETCH_CASES, ids=lambda c: 'M%d' % c[1])
def test_attn_fwd_value_prefetch_boundary(case, use_mask):
    """M = 28 takes the value-prefetch path of attn_fwd_kernel (Cv = 2048), M = 29 the channel loop"""
    assert lib().comic_attn_splits(case[0], case[1]) == 1
    f = fwd_case(case, use_mask)
    check_fwd(f, launch_fwd(f, scratch=True), 'M=%d:' % case[1])


def test_attn_fwd_channel_share_wider_than_the_workgroup():
    """Cv = 4096 at S = 2: ceil(Cv / S) = 2048 channels per workgroup of 1024 threads.  attn_ctx_kernel writes one channel
    per thread, so the split form used to return 0 with half of ctx unwritten; the library now takes the one-workgroup
    form (which loops over the channels) for such shapes."""
    case = R.HOLE_CASE
    assert lib().comic_attn_splits(case[0], case[1]) == 2
    f = fwd_case(case, False)
    check_fwd(f, launch_fwd(f, scratch=True), 'Cv=4096 with scratch:')


@pytest.mark.parametrize('q_parts', [2, 5, 6])
@pytest.mark.parametrize('scratch', [False, True])
@pytest.mark.parametrize('case', R.EPILOGUE_CASES, ids=lambda c: 'x'.join(map(str, c[:5])))
def test_attn_fwd_fused_epilogue(case, scratch, q_parts):
    run_fused_epilogue(case, scratch, q_parts)


@pytest.mark.parametrize('regime', ATTN_REGIMES, ids=str)
def test_attn_fwd_fused_epilogue_off_unit_scale(regime):
    run_fused_epilogue(R.EPILOGUE_CASES[0], False, 5, regime)


def run_fused_epilogue(case, scratch, q_parts, regime=None):
    """lens / t / att_prev -> att_next, xh_next at a column offset of wider rows under mask_next / keep_in, q from its
    split-K partials (sum_q_parts: four slices at a time + remainder) and q_out.  Measured on an MI355X: q_out is
    bit-equal to the float32 sum in slice order in all twelve cases (asserted at 1e-6, as the kernel may re-associate)"""
    B, M, D, H, Cv = case[:5]
    S = lib().comic_attn_splits(B, M) if scratch else 1
    assert S == (8 if (scratch and M >= 49) else 1)
    f = fwd_case(case, True, 1, regime)
    e = ew(regime)
    rng = np.random.default_rng(q_parts)
    parts = rng.standard_normal((q_parts, B, D)).astype(np.float32)
    parts[0] = f.inp['q'] - parts[1:].sum(0)                         # the partials add up to (about) the case's q
    q32 = parts[0].copy()
    for s in range(1, q_parts):
        q32 = q32 + parts[s]                                         # float32, slice order
    lens = np.array([3, 1, 5, 2, 9][:B], np.int32)
    t, keep_in = 2, 0.8
    fin = t >= lens
    assert fin.any() and not fin.all()
    att_prev = rng.standard_normal((B, Cv)).astype(np.float32)
    xh_ld, xh_off, mask_ld, mask_off = Cv + 40, 24, Cv + 8, 4
    mask_next = (rng.random((B, mask_ld)) < keep_in).astype(np.float32)
    alpha_r, alpha_d_r, ctx_r, _ = R.attn_fwd_ref(case, f.inp['keys'], f.inp['values'], q32, f.inp['p'], f.mask, f.keep)
    att_next_r, xh_r = R.epilogue_ref(ctx_r, att_prev.astype(np.float64), lens, t,
                                      mask_next[:, mask_off:mask_off + Cv].astype(np.float64), keep_in)
    d_lens, d_prev, d_mask, d_parts = dev(lens), dev(att_prev), dev(mask_next), dev(parts)
    att_next, xh, q_out = nan(B, Cv), nan(B, xh_ld), nan(B, D)
    rc, alpha, alpha_d, ctx = launch_fwd(f, scratch, q=d_parts, q_parts=q_parts, q_out=q_out, lens=d_lens, t=t,
                                         att_prev=d_prev, att_next=att_next, xh_next=ptr(xh, xh_off), xh_ld=xh_ld,
                                         mask_next=ptr(d_mask, mask_off), mask_ld=mask_ld, keep_in=keep_in)
    assert rc == 0, lib().comic_last_error()
    print('  q_out bit-equal to the float32 sum in slice order: %s' % bool(np.array_equal(host(q_out), q32)))
    chk('q_out', q_out, q32, 1e-6)
    chk('alpha', alpha, alpha_r, R.ATTN_FWD_TOL, e)
    chk('alpha_d', alpha_d, alpha_d_r, R.ATTN_FWD_TOL, e)
    chk('ctx', ctx, ctx_r, R.ATTN_FWD_TOL, e)
    chk('att_next', att_next, att_next_r, R.ATTN_FWD_TOL, e)
    np.testing.assert_array_equal(host(att_next)[fin], att_prev[fin])            # finished rows: the previous state, exactly
    np.testing.assert_array_equal(host(att_next)[~fin], host(ctx)[~fin])
    xh_h = host(xh)
    chk('xh_next', xh_h[:, xh_off:xh_off + Cv], xh_r, R.ATTN_FWD_TOL, e)
    assert np.isnan(xh_h[:, :xh_off]).all() and np.isnan(xh_h[:, xh_off + Cv:]).all(), 'xh_next written outside its columns'
    # the pre-summed q in one slice gives the same step
    rc, alpha1, alpha_d1, ctx1 = launch_fwd(f, scratch, q=dev(q32))
    assert rc == 0
    chk('alpha vs pre-summed q', alpha, host(alpha1), R.ATTN_FWD_TOL)
    chk('ctx vs pre-summed q', ctx, host(ctx1), R.ATTN_FWD_TOL)


MEM_DIV_CASES = [  # entries, W, M, D, H, Cv, method, tied, scratch
    (1, 3, 9, 64, 2, 64, 'dot', True, False), (3, 3, 9, 64, 2, 64, 'dot', True, False),
    (8, 2, 9, 64, 2, 64, 'dot', True, False), (9, 5, 9, 64, 2, 64, 'dot', True, False),
    (17, 2, 9, 64, 2, 64, 'dot', True, False),
    (3, 3, 25, 512, 8, 2048, 'add_LN', False, False),          # value-prefetch path
    (3, 3, 64, 64, 2, 64, 'dot', True, True)]                  # split form


@pytest.mark.parametrize('mc', MEM_DIV_CASES, ids=lambda m: 'e%dxW%d_M%d' % m[:3])
def test_attn_fwd_shared_memories(mc):
    """mem_div = W: the beams of an entry share one copy of the keys / values (grid rounded up to 8 W, workgroup ->
    (entry, beam) map); the reference repeats the memories W times"""
    entries, W, M, D, H, Cv, method, tied, scratch = mc
    case = (entries * W, M, D, H, Cv, method, 'softmax', tied)
    assert lib().comic_attn_splits(case[0], M) == (8 if scratch else 1)
    f = fwd_case(case, True, W)
    check_fwd(f, launch_fwd(f, scratch), 'mem_div=%d:' % W)


@pytest.mark.parametrize('regime', ATTN_REGIMES, ids=str)
def test_attn_fwd_shared_memories_off_unit_scale(regime):
    """mem_div = 3 on the add_LN entry of MEM_DIV_CASES"""
    entries, W, M, D, H, Cv, method, tied, scratch = MEM_DIV_CASES[5]
    assert (W, method) == (3, 'add_LN')
    f = fwd_case((entries * W, M, D, H, Cv, method, 'softmax', tied), True, W, regime)
    check_fwd(f, launch_fwd(f, scratch), '%s mem_div=%d:' % (regime, W))


def test_attn_fwd_shared_memories_refuse_a_ragged_batch():
    case = (9, 9, 64, 2, 64, 'dot', 'softmax', True)
    f = fwd_case(case, False, 3)
    rc = launch_fwd(f, False, B=7)[0]
    assert rc != 0 and b'multiple' in lib().comic_last_error()


# ============================================================================ attention, backward ====================
class Bwd:
    def __init__(self, case, with_dmap=True, with_lens=True, regime=None):
        B, M, D, H, Cv, method, prob, tied = case
        f = self.f = fwd_case(case, True, 1, regime)
        rng = np.random.default_rng(B + M + D)
        self.dctx = rng.standard_normal((B, Cv)).astype(np.float32)
        self.dmap = (0.01 * rng.standard_normal((B, M))).astype(np.float32) if with_dmap else None
        self.t = 2
        self.lens = np.array([3, 1, 5, 2, 9, 2, 4] * ((B + 6) // 7), np.int32)[:B] if with_lens else None
        # the kernel's alpha operand: the float32 rounding of the reference probabilities
        self.alpha32 = f.alpha.astype(np.float32)
        self.ref = R.attn_bwd_ref(case, f.inp['keys'], f.inp['values'], f.inp['q'], f.inp['p'], f.mask, f.keep, self.dctx,
                                  self.dmap, self.lens, self.t)
        self.pre_k = (0.01 * rng.standard_normal((B, M, D))).astype(np.float32)
        self.pre_v = (0.01 * rng.standard_normal((B, M, Cv))).astype(np.float32)
        self.pre_pg = (0.01 * rng.standard_normal((B, 3 * D + 1))).astype(np.float32)
        self.d_alpha, self.d_dctx = dev(self.alpha32), dev(self.dctx)
        self.d_dmap = dev(self.dmap) if with_dmap else None
        self.d_lens = dev(self.lens) if with_lens else None


@functools.lru_cache(maxsize=2)
def bwd_case(case, with_dmap=True, with_lens=True, regime=None):
    return Bwd(case, with_dmap, with_lens, regime)


BWD_MODES = {'add': (0, False), 'overwrite': (1, False), 'split2': (2, False), 'split_scratch': (2, True)}


def launch_bwd(b, mode):
    """-> rc, dq, dkeys, dvalues (None when tied), pgrad"""
    f = b.f
    B, M, D, H, Cv, method, prob, tied = f.case
    over, scratch = BWD_MODES[mode]
    d = desc(f.case)
    dq = torch.zeros((B, D), device=DEV) if over == 2 else nan(B, D)
    pgrad = dev(b.pre_pg) if over == 0 else (torch.zeros((B, 3 * D + 1), device=DEV) if over == 2 else nan(B, 3 * D + 1))
    dkeys = dev(b.pre_k)
    dvalues = None if tied else dev(b.pre_v)
    ws_s = nan(B * H * M) if scratch else None
    ws_d = nan(int(lib().comic_attn_bwd_scratch(B, H, M, D))) if scratch else None
    rc = lib().comic_op_attn_bwd(C.byref(d), ptr(f.d_keys), ptr(f.d_values), ptr(f.d_q), ptr(f.d_p['ln_g']), ptr(f.d_p['ln_b']),
                                 ptr(f.d_p['v']), ptr(f.d_p['tau']), ptr(b.d_alpha), ptr(f.d_mask), f.keep, ptr(b.d_dctx),
                                 ptr(b.d_dmap), ptr(dq), ptr(dkeys), ptr(dkeys if tied else dvalues), ptr(pgrad),
                                 ptr(b.d_lens), b.t, over, ptr(ws_s), ptr(ws_d), stream())
    sync()
    return rc, dq, dkeys, dvalues, pgrad


def check_bwd(b, mode, out):
    B, M, D, H, Cv, method, prob, tied = b.f.case
    rc, dq, dkeys, dvalues, pgrad = out
    over = BWD_MODES[mode][0]
    assert rc == 0, lib().comic_last_error()
    ref = b.ref
    chk(mode + ' dq', dq, ref['dq'], F32_RTOL)
    # d keys / d values accumulate: what the launch added to the prefill
    if tied:
        chk(mode + ' dkeys(tied) - prefill', host(dkeys).astype(np.float64) - b.pre_k, ref['dkeys'] + ref['dvalues'], F32_RTOL)
    else:
        chk(mode + ' dkeys - prefill', host(dkeys).astype(np.float64) - b.pre_k, ref['dkeys'], F32_RTOL)
        chk(mode + ' dvalues - prefill', host(dvalues).astype(np.float64) - b.pre_v, ref['dvalues'], F32_RTOL)
    pg = host(pgrad).astype(np.float64)
    if method != 'add_LN':              # no parameters: the rows are left alone
        np.testing.assert_array_equal(host(pgrad), b.pre_pg if over == 0 else (np.zeros_like(b.pre_pg) if over == 2 else
                                                                              np.full_like(b.pre_pg, NAN)))
        return
    if over == 0:                       # adds to the prefill
        pg = pg - b.pre_pg
    for name, lo, hi in (('dv', 0, D), ('dln_g', D, 2 * D), ('dln_b', 2 * D, 3 * D), ('dtau', 3 * D, 3 * D + 1)):
        chk('%s pgrad rows %s' % (mode, name), pg[:, lo:hi], ref['pgrad'][:, lo:hi], F32_RTOL)


@pytest.mark.parametrize('mode', list(BWD_MODES))
@pytest.mark.parametrize('case,S', R.BWD_CASES, ids=lambda v: 'x'.join(map(str, v[:5])) if isinstance(v, tuple) else 'S%d' % v)
def test_attn_bwd_forms(case, S, mode):
    """pgrad_overwrite 0 (adds to a prefilled row), 1 (overwrites NaN), 2 without scratch (two workgroups, atomic adds into
    zero-filled rows) and 2 with scratch (S > 2: attn_bwd_scores_kernel -> attn_bwd_kernel partial rows ->
    attn_bwd_reduce_kernel; S <= 2: the two-workgroup form), with an alpha dropout mask, finished rows (live = 0: no d ctx
    passes, dmap still does) and accumulating d keys / d values"""
    B, M, D, H, Cv, method, prob, tied = case
    assert lib().comic_attn_splits(B, M) == S
    over, scratch = BWD_MODES[mode]
    b = bwd_case(case)
    assert (b.t >= b.lens).any() and (b.t < b.lens).any()
    out = launch_bwd(b, mode)
    if over == 2 and prob == 'sigmoid':
        assert out[0] != 0 and b'softmax' in lib().comic_last_error()     # the split form recomputes only its own scores
        return
    check_bwd(b, mode, out)
    if over == 2:       # two addends commute; the S > 2 partial rows are reduced in a fixed order: the same bits every time
        again = launch_bwd(b, mode)
        for name, x, y in zip(('dq', 'dkeys', 'dvalues', 'pgrad'), out[1:], again[1:]):
            assert x is None or torch.equal(x, y), '%s %s: two launches differ' % (mode, name)


@pytest.mark.parametrize('regime', ATTN_REGIMES, ids=str)
@pytest.mark.parametrize('mode', ['add', 'overwrite', 'split2'])
def test_attn_bwd_forms_off_unit_scale(mode, regime):
    """pgrad_overwrite 0, 1, 2 on the smallest add_LN softmax case of test_attn_bwd_forms (the split form refuses
    sigmoid).  The backward re-derives mean and 1 / std of keys + q in two passes; at gains x 40 most of 1 - tanh^2 is an
    exact zero, so the gradients are held element-wise as well"""
    case, S = R.BWD_CASES[-1]
    assert lib().comic_attn_splits(case[0], case[1]) == S == 1
    b = bwd_case(case, True, True, regime)
    out = launch_bwd(b, mode)
    check_bwd(b, mode, out)
    assert all(x is None or bool(torch.isfinite(x).all()) for x in out[1:])


@pytest.mark.parametrize('mode', ['overwrite', 'split_scratch'])
@pytest.mark.parametrize('case', [R.BWD_CASES[0][0], R.BWD_CASES[-1][0]], ids=lambda c: 'x'.join(map(str, c[:5])))
def test_attn_bwd_without_map_loss_and_lens(case, mode):
    """dmap may be NULL (no map loss) and lens may be NULL (every row live)"""
    b = bwd_case(case, False, False)
    check_bwd(b, mode, launch_bwd(b, mode))


# ============================================================================ losses ================================
XENT_GEOM = [  # t_rows, t_stride, B, H, M  ->  n = t_rows*B*M map elements
    (5, 7, 3, 2, 5),            # 75: one piece
    (5, 7, 3, 2, 20),           # 300: two pieces, the second ragged
    (7, 9, 48, 8, 196)]         # 65856: 258 pieces, more than one pass of the final 256-thread sum


def xent_operands(V, t_rows, t_stride, B, rng, regime=None):
    if regime is not None:
        assert regime == 'peaked', regime
        return R.xent_operands_peaked(V, t_rows, t_stride, B, rng)
    logits = (3 * rng.standard_normal((t_rows, B, V))).astype(np.float32)
    lens = rng.integers(1, t_stride + 1, B).astype(np.int32)
    lens[:3] = (t_rows, 3, t_stride)
    targets = rng.integers(0, V, (B, t_stride)).astype(np.int32)
    wmask = (np.arange(t_stride)[None, :] < lens[:, None]).astype(np.float32)
    coef = (wmask / wmask.sum()).astype(np.float32)
    return logits, lens, targets, wmask, coef


def check_xent(V, t_rows, B, ops, d_logits, loss_rows, dlog, ids, ld_dl, regime=None):
    logits, lens, targets, wmask, coef = ops
    lg, xent, dl_ref, amax = R.xent_ref(logits, targets, coef, wmask, lens)
    np.testing.assert_array_equal(host(d_logits), lg)                           # finished rows zeroed in place
    # element-wise too: a max-norm relative to the largest loss row (230 in the peaked regime) hides the small rows
    chk('xent rows', host(loss_rows).reshape(t_rows, B), xent, R.XENT_TOL, True)
    dl = host(dlog).reshape(t_rows, B, ld_dl)
    chk('dlogits', dl[..., :V], dl_ref, R.XENT_TOL, ew(regime))
    assert (dl[..., V:] == 0).all(), 'padding columns of d logits are not exactly zero'
    np.testing.assert_array_equal(host(ids).reshape(t_rows, B), amax)


@pytest.mark.parametrize('with_dmap', [True, False])
@pytest.mark.parametrize('geom', XENT_GEOM, ids=lambda g: 'n%d' % (g[0] * g[2] * g[4]))
@pytest.mark.parametrize('V', [258, 1000])
def test_xent_maploss(V, geom, with_dmap):
    run_xent_maploss(V, geom, with_dmap)


def test_xent_maploss_peaked_logits():
    """logit rows 30 N(0,1) +- 200 with a dominant entry: an all-equal row, a target that is the arg-max (loss below
    float32 epsilon) and a target whose probability underflows (loss 150, finite)"""
    run_xent_maploss(258, XENT_GEOM[0], True, 'peaked')


def run_xent_maploss(V, geom, with_dmap, regime=None):
    """xent_maploss_kernel: the sequence loss with ld_dl > V and the attention-map loss in one launch; the last-arriver
    ticket is zero again afterwards, so a second launch needs no re-zeroing and gives the same bits"""
    t_rows, t_stride, B, H, M = geom
    rng = np.random.default_rng(V + M)
    ops = xent_operands(V, t_rows, t_stride, B, rng, regime)
    logits, lens, targets, wmask, coef = ops
    hist = (rng.random((t_rows, B, H, M)) * (2.0 / H)).astype(np.float32)
    scale, ld_dl = 0.7, V + 6
    n = t_rows * B * M
    nparts = (n + 255) // 256
    loss_ref, dmap_ref = R.map_loss_ref(hist, scale)
    d_logits, d_hist = dev(logits), dev(hist)
    d_t, d_c, d_w, d_l = dev(targets), dev(coef), dev(wmask), dev(lens)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    runs = []
    for _ in range(2):
        loss_rows, dlog = nan(t_rows * B), nan(t_rows * B, ld_dl)
        ids = torch.full((t_rows, B), -1, dtype=torch.int32, device=DEV)
        dmap = nan(t_rows, B, M) if with_dmap else None
        partial, map_loss = nan(nparts), nan(1)
        L.check(lib().comic_op_xent_maploss(ptr(d_logits), ptr(d_t), ptr(d_c), ptr(d_w), ptr(d_l), ptr(loss_rows), ptr(dlog),
                                            ld_dl, ptr(ids), t_rows, t_stride, B, V, ptr(d_hist), ptr(dmap), ptr(partial),
                                            ptr(map_loss), ptr(ticket), H, M, scale, stream()), 'xent_maploss')
        sync()
        assert int(ticket.item()) == 0, 'the ticket is not zero after the launch'
        runs.append((loss_rows, dlog, ids, dmap, map_loss))
    loss_rows, dlog, ids, dmap, map_loss = runs[0]
    check_xent(V, t_rows, B, ops, d_logits, loss_rows, dlog, ids, ld_dl, regime)
    chk('map_loss', map_loss, [loss_ref], R.XENT_TOL)
    if with_dmap:
        chk('dmap', dmap, dmap_ref, R.XENT_TOL)
    for x, y in zip(runs[0], runs[1]):
        assert x is None or torch.equal(x, y), 'two launches in a row differ'


@pytest.mark.parametrize('V', [258, 1000])
def test_xent_fewer_rows_than_the_table_stride(V):
    run_xent_fewer_rows(V)


def test_xent_peaked_logits():
    run_xent_fewer_rows(258, 'peaked')


def run_xent_fewer_rows(V, regime=None):
    """comic_xent_ex with t_rows < t_stride: the [B, t_stride] tables are indexed b*t_stride + t"""
    t_rows, t_stride, B = 5, 7, 3
    ops = xent_operands(V, t_rows, t_stride, B, np.random.default_rng(V), regime)
    logits, lens, targets, wmask, coef = ops
    d_logits = dev(logits)
    loss_rows, dlog = nan(t_rows * B), nan(t_rows * B, V)
    ids = torch.full((t_rows, B), -1, dtype=torch.int32, device=DEV)
    L.check(lib().comic_op_xent(ptr(d_logits), P(targets), P(coef), P(wmask), P(lens),
                                ptr(loss_rows), ptr(dlog), ptr(ids), t_rows, t_stride, B, V, stream()), 'xent')
    sync()
    check_xent(V, t_rows, B, ops, d_logits, loss_rows, dlog, ids, V, regime)


# ============================================================================ LN_LSTM ===============================
CELL_B, CELL_LENS, CELL_T, KEEP_OUT = 5, np.array([3, 1, 5, 2, 9], np.int32), 2, 0.65


def partials(rng, S, *shape):
    return (rng.standard_normal((S,) + shape) / np.sqrt(S)).astype(np.float32)


@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('D', R.LN_LSTM_D)
def test_ln_lstm_fwd_bwd(D, S):
    run_ln_lstm(D, S)


@pytest.mark.parametrize('regime', LN_LSTM_REGIMES, ids=str)
@pytest.mark.parametrize('D', [128, 512])
def test_ln_lstm_off_unit_scale(D, regime):
    """the four gate rows and the cell row with a mean of 4 and 8 standard deviations (R.ln_lstm_regime), and the five
    gains x 40 with cell states to +-50: pre-activations beyond +-100, tanh(c) = +-1"""
    run_ln_lstm(D, 3, regime)


def run_ln_lstm(D, S, regime=None):
    """PER = 1, 2, 4, 8 units per thread with the last 256-chunk full and partial (d < D guards), S split-K partials,
    finished rows, output dropout, h into the next operand row at an offset, and NULL previous states"""
    B, t, lens = CELL_B, CELL_T, CELL_LENS
    rng = np.random.default_rng(D + S)
    ls = lib().comic_cell_ln_stride(D)
    assert ls == (D + 63) // 64 * 64 and (D != 100 or ls == 128)
    g = partials(rng, S, B, 4 * D)
    ln = R.ln_params(rng, D)
    ln_dev = np.full((10, ls), NAN, np.float32)
    ln_dev[:, :D] = ln
    mask = (rng.random((B, D)) < KEEP_OUT).astype(np.float32)
    fin = t >= lens
    live = (~fin)[:, None].astype(np.float64)
    xh_ld, xh_off = D + 24, 8
    d_mask, d_lens = dev(mask), dev(lens)
    g0, ln0, e = g, ln, ew(regime)
    for null_state in (False, True):
        tag = 'D=%d S=%d%s%s ' % (D, S, ' null state' if null_state else '', '' if regime is None else ' %s' % (regime,))
        c = None if null_state else rng.standard_normal((B, D)).astype(np.float32)
        h = None if null_state else rng.standard_normal((B, D)).astype(np.float32)
        if regime is not None:
            g, c, ln = R.ln_lstm_regime(g0, c, ln0, regime)
            ln_dev[:, :D] = ln
        d_g, d_ln = dev(g), dev(ln_dev)
        fw = R.ln_lstm_fwd_ref(R.f64(g).sum(0), ln, c)
        rs = dict.fromkeys(fw)
        if regime is not None:                                  # the float32 restatement (partials added in the kernel's order)
            g32 = g[0]
            for k in range(1, S):
                g32 = g32 + g[k]
            with np.errstate(over='ignore'):
                rs = {k: G.rel_err(v, fw[k]) for k, v in R.ln_lstm_fwd_ref(g32, ln, c, dtype=np.float32).items()}
        d_c, d_h = (None, None) if null_state else (dev(c), dev(h))
        ga, xhat, rstd, c_new, y = nan(B, 4 * D), nan(B, 5 * D), nan(B, 8), nan(B, D), nan(B, D)
        cs, hs, xh = nan(B, D), nan(B, D), nan(B, xh_ld)
        L.check(lib().comic_op_ln_lstm_fwd(ptr(d_g), S, ptr(d_ln), ptr(d_c), ptr(d_h), ptr(ga), ptr(xhat), ptr(rstd), ptr(c_new),
                                           ptr(y), ptr(d_mask), KEEP_OUT, ptr(d_lens), t, ptr(cs), ptr(hs), B, D,
                                           ptr(xh, xh_off), xh_ld, stream()), 'ln_lstm_fwd')
        sync()
        hs_ref = R.state_select(fin, R.f64(h), fw['h_new'])
        chk(tag + 'gates_act', ga, fw['gates_act'], R.GATES_TOL, e, rs['gates_act'])
        chk(tag + 'xhat', xhat, fw['xhat'], R.GATES_TOL, e, rs['xhat'])
        chk(tag + 'rstd', host(rstd)[:, :5], fw['rstd'], R.GATES_TOL, e, rs['rstd'])
        chk(tag + 'c_new', c_new, fw['c_new'], R.GATES_TOL, e, rs['c_new'])
        chk(tag + 'y', y, dr.dropout(fw['h_new'], R.f64(mask), KEEP_OUT), R.GATES_TOL, e, rs['h_new'])
        chk(tag + 'c_state', cs, R.state_select(fin, R.f64(c), fw['c_new']), R.GATES_TOL, e, rs['c_new'])
        chk(tag + 'h_state', hs, hs_ref, R.GATES_TOL, e, rs['h_new'])
        xh_h = host(xh)
        chk(tag + 'xh_next', xh_h[:, xh_off:xh_off + D], hs_ref, R.GATES_TOL, e, rs['h_new'])
        assert np.isnan(xh_h[:, :xh_off]).all() and np.isnan(xh_h[:, xh_off + D:]).all()
        # ---- backward on the float32 roundings of the reference's saved tensors ----
        f32 = {k: v.astype(np.float32) for k, v in fw.items()}
        rstd8 = np.full((B, 8), NAN, np.float32)
        rstd8[:, :5] = f32['rstd']
        dy = rng.standard_normal((B, D)).astype(np.float32)
        dyp = partials(rng, S, B, D)
        dc = rng.standard_normal((B, D)).astype(np.float32)
        dh = rng.standard_normal((B, D)).astype(np.float32)
        dh2 = R.f64(dh) * live + dr.dropout(R.f64(dy) + R.f64(dyp).sum(0), R.f64(mask), KEEP_OUT)
        dg_ref, rows_ref, dcp_ref = R.ln_lstm_bwd_ref({k: R.f64(v) for k, v in f32.items()}, ln, c, R.f64(dc) * live, dh2)
        d_dc, d_dh, dg, pg = dev(dc), dev(dh), nan(B, 4 * D), nan(B, 10, D)
        L.check(lib().comic_op_ln_lstm_bwd(P(f32['gates_act']), P(f32['xhat']), P(rstd8), ptr(d_ln), ptr(d_c),
                                           P(f32['c_new']), P(dy), P(dyp), S, ptr(d_mask), KEEP_OUT,
                                           ptr(d_lens), t, ptr(d_dc), ptr(d_dh), ptr(dg), ptr(pg), B, D, stream()), 'ln_lstm_bwd')
        sync()
        chk(tag + 'dg', dg, dg_ref, F32_RTOL)
        for k in range(10):
            chk(tag + 'ln row %d' % k, host(pg)[:, k], rows_ref[:, k], F32_RTOL)
        chk(tag + 'dc', d_dc, R.f64(dc) * (1 - live) + dcp_ref, F32_RTOL)
        chk(tag + 'dh', d_dh, R.f64(dh) * (1 - live), F32_RTOL)


def test_ln_lstm_refuses_more_than_2048_units():
    B, D = 1, 2049
    z = torch.zeros(B * 10 * 2112, device=DEV)        # every operand fits, should the check ever be lost
    il = torch.ones(B, dtype=torch.int32, device=DEV)
    p = ptr(z)
    assert lib().comic_op_ln_lstm_fwd(p, 1, p, p, p, p, p, p, p, p, p, 1.0, ptr(il), 0, p, p, B, D, p, D, stream()) != 0
    assert b'2049' in lib().comic_last_error()
    assert lib().comic_op_ln_lstm_bwd(p, p, p, p, p, p, p, p, 1, p, 1.0, ptr(il), 0, p, p, p, p, B, D, stream()) != 0
    sync()


@pytest.mark.parametrize('D', [64, 100, 2048])
def test_ln_lstm_scatter(D):
    ls = lib().comic_cell_ln_stride(D)
    rng = np.random.default_rng(D)
    sums = rng.standard_normal((10, D)).astype(np.float32)
    pre = rng.standard_normal((10, ls)).astype(np.float32)
    out0, out1 = nan(10, ls), dev(pre)
    L.check(lib().comic_op_ln_lstm_scatter(P(sums), ptr(out0), D, 0.0, stream()))
    L.check(lib().comic_op_ln_lstm_scatter(P(sums), ptr(out1), D, 1.0, stream()))
    sync()
    np.testing.assert_array_equal(host(out0)[:, :D], sums)
    assert np.isnan(host(out0)[:, D:]).all()
    chk('scatter beta 1', host(out1)[:, :D], R.f64(pre[:, :D]) + sums, 1e-6)
    np.testing.assert_array_equal(host(out1)[:, D:], pre[:, D:])


# ============================================================================ GRU ===================================
@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('EA', [64 + 192, 100])
@pytest.mark.parametrize('D', R.GRU_D)
def test_gru_kernels(D, EA, S):
    run_gru(D, EA, S)


def test_gru_kernels_saturated():
    """the smallest test_gru_kernels case with both products scaled to reach +-100: expf(-x) is inf, r (1 - r) and
    1 - cand^2 are exact zeros almost everywhere; forward and gradients held element-wise"""
    run_gru(R.GRU_D[0], 64 + 192, 1, 'saturated')


def run_gru(D, EA, S, regime=None):
    """gru_gates_fwd / gru_out_fwd / gru_bwd1 / gru_bwd2 on their own operands, padded leading dimensions, finished
    rows and a NULL previous state"""
    B, t, lens = CELL_B, CELL_T, CELL_LENS
    rng = np.random.default_rng(D + EA + S)
    Wd = EA + D
    fin = t >= lens
    live = (~fin)[:, None].astype(np.float64)
    g1, g2 = partials(rng, S, B, 2 * D), partials(rng, S, B, D)
    b_g = (1 + 0.1 * rng.standard_normal(2 * D)).astype(np.float32)
    b_c = (0.1 * rng.standard_normal(D)).astype(np.float32)
    e = ew(regime)
    if regime is not None:
        assert regime == 'saturated', regime
        g1, g2 = G.saturate_partials(g1, b_g), G.saturate_partials(g2, b_c)
    xh_ld, ld_ru, xh2_ld, ld_cand, ld_dpre, xn_ld, xn_off = Wd + 8, 2 * D + 4, Wd + 16, D + 12, 3 * D + 4, Wd + 8, EA
    xh_in = rng.standard_normal((B, xh_ld)).astype(np.float32)
    mask = (rng.random((B, D)) < KEEP_OUT).astype(np.float32)
    d_lens, d_mask = dev(lens), dev(mask)
    for null_state in (False, True):
        tag = 'D=%d EA=%d S=%d%s ' % (D, EA, S, ' null h' if null_state else '')
        h = None if null_state else rng.standard_normal((B, D)).astype(np.float32)
        h64 = np.zeros((B, D)) if null_state else R.f64(h)
        d_h = None if null_state else dev(h)
        r, u, cand, h_new = R.gru_fwd_ref(R.f64(g1).sum(0), b_g, lambda rh: R.f64(g2).sum(0), b_c, h)
        ru, xh2 = nan(B, ld_ru), nan(B, xh2_ld)
        L.check(lib().comic_op_gru_gates_fwd(P(g1), S, P(b_g), ptr(d_h), P(xh_in), xh_ld, ptr(ru), ld_ru,
                                             ptr(xh2), xh2_ld, B, D, EA, stream()), 'gru_gates_fwd')
        sync()
        ru_h, xh2_h = host(ru), host(xh2)
        chk(tag + 'ru', ru_h[:, :2 * D], np.concatenate([r, u], 1), R.GATES_TOL, e)
        assert np.isnan(ru_h[:, 2 * D:]).all() and np.isnan(xh2_h[:, Wd:]).all()
        np.testing.assert_array_equal(xh2_h[:, :EA], xh_in[:, :EA])                 # the x / att columns: a copy
        chk(tag + 'xh2 r*h', xh2_h[:, EA:Wd], r * h64, R.GATES_TOL, e)
        # candidate + new state, on the float32 rounding of the reference gates
        ru32 = np.full((B, ld_ru), NAN, np.float32)
        ru32[:, :D], ru32[:, D:2 * D] = r, u
        u32 = R.f64(ru32[:, D:2 * D])
        h_new = u32 * h64 + (1 - u32) * cand
        hs_ref = np.where(fin[:, None], h64, h_new)
        cand_o, y, hs, xn = nan(B, ld_cand), nan(B, D), nan(B, D), nan(B, xn_ld)
        d_ru = dev(ru32)
        L.check(lib().comic_op_gru_out_fwd(P(g2), S, P(b_c), ptr(d_ru), ld_ru, ptr(d_h), ptr(cand_o), ld_cand, ptr(y),
                                           ptr(d_mask), KEEP_OUT, ptr(d_lens), t, ptr(hs), ptr(xn, xn_off), xn_ld, B, D,
                                           stream()), 'gru_out_fwd')
        sync()
        chk(tag + 'cand', host(cand_o)[:, :D], cand, R.GATES_TOL, e)
        assert np.isnan(host(cand_o)[:, D:]).all()
        chk(tag + 'y', y, dr.dropout(h_new, R.f64(mask), KEEP_OUT), R.GATES_TOL, e)
        chk(tag + 'h_state', hs, hs_ref, R.GATES_TOL, e)
        chk(tag + 'xh_next', host(xn)[:, xn_off:xn_off + D], hs_ref, R.GATES_TOL, e)
        assert np.isnan(host(xn)[:, :xn_off]).all() and np.isnan(host(xn)[:, xn_off + D:]).all()
        # ---- backward ----
        cand32 = np.full((B, ld_cand), NAN, np.float32)
        cand32[:, :D] = cand
        dy = rng.standard_normal((B, D)).astype(np.float32)
        dyp = partials(rng, S, B, D)
        dh = rng.standard_normal((B, D)).astype(np.float32)
        dxh2 = rng.standard_normal((B, xh2_ld)).astype(np.float32)
        dh2 = R.f64(dh) * live + dr.dropout(R.f64(dy) + R.f64(dyp).sum(0), R.f64(mask), KEEP_OUT)
        r32 = R.f64(ru32[:, :D])
        dpc, dpu, dpr, dh_u, dh_r = R.gru_bwd_ref(r32, u32, R.f64(cand32[:, :D]), h64, dh2, R.f64(dxh2[:, EA:Wd]))
        d_dh, dpre, d_dxh2, d_cand = dev(dh), nan(B, ld_dpre), dev(dxh2), dev(cand32)
        L.check(lib().comic_op_gru_bwd1(P(dy), P(dyp), S, ptr(d_mask), KEEP_OUT, ptr(d_lens), t, ptr(d_dh), ptr(d_ru),
                                        ld_ru, ptr(d_cand), ld_cand, ptr(d_h), ptr(dpre), ld_dpre, B, D, stream()), 'gru_bwd1')
        L.check(lib().comic_op_gru_bwd2(ptr(d_dxh2), xh2_ld, ptr(d_ru), ld_ru, ptr(d_h), ptr(dpre), ld_dpre, B, D, EA, stream()),
                'gru_bwd2')
        sync()
        dpre_h, dx_h = host(dpre), host(d_dxh2)
        if null_state:                    # h = 0: d r_pre is exactly zero, which the relative measures cannot divide by
            assert (dpre_h[:, :D] == 0).all()
        else:
            chk(tag + 'dpre r', dpre_h[:, :D], dpr, F32_RTOL)
        chk(tag + 'dpre u', dpre_h[:, D:2 * D], dpu, F32_RTOL)
        chk(tag + 'dpre cand', dpre_h[:, 2 * D:3 * D], dpc, F32_RTOL)
        assert np.isnan(dpre_h[:, 3 * D:]).all()
        chk(tag + 'dh_state', d_dh, R.f64(dh) * (1 - live) + dh_u, F32_RTOL)
        chk(tag + 'dxh2 h third', dx_h[:, EA:Wd], dh_r, F32_RTOL)
        np.testing.assert_array_equal(dx_h[:, :EA], dxh2[:, :EA])
        np.testing.assert_array_equal(dx_h[:, Wd:], dxh2[:, Wd:])


# ============================================================================ LSTM gates, executor form =============
@pytest.mark.parametrize('D', [128, 100])
def test_lstm_gates_split_k_partials_and_bias(D):
    run_lstm_gates_split_k(D)


def test_lstm_gates_saturated():
    """comic_lstm_gates_fwd / _bwd and the executor forms with pre-activations to +-100 and cell states to +-50"""
    run_lstm_gates_split_k(128, 'saturated')


def run_lstm_gates_split_k(D, regime=None):
    """S = 3 partials + bias / dy_part / xh_next: the public op on the pre-summed, biased product gives the same step"""
    B, S, t, lens = 6, 3, 2, np.array([3, 1, 5, 2, 9, 2], np.int32)
    rng = np.random.default_rng(D)
    g = partials(rng, S, B, 4 * D)
    bias = (0.1 * rng.standard_normal(4 * D)).astype(np.float32)
    c = rng.standard_normal((B, D)).astype(np.float32)
    h = rng.standard_normal((B, D)).astype(np.float32)
    mask = (rng.random((B, D)) < KEEP_OUT).astype(np.float32)
    fin = t >= lens
    e = ew(regime)
    if regime is not None:
        assert regime == 'saturated', regime
        g, c = G.saturate_partials(g, bias), G.saturate(c, G.CELL_PEAK)
    g32 = ((g[0] + g[1]) + g[2]) + bias                       # float32, the kernel's order
    xh_ld, xh_off = D + 24, 8
    d_c, d_h, d_mask, d_lens = dev(c), dev(h), dev(mask), dev(lens)
    ex = dict(ga=nan(B, 4 * D), c_new=nan(B, D), y=nan(B, D), cs=nan(B, D), hs=nan(B, D))
    pub = dict(ga=nan(B, 4 * D), c_new=nan(B, D), y=nan(B, D), cs=nan(B, D), hs=nan(B, D))
    xh, h_new = nan(B, xh_ld), nan(B, D)
    L.check(lib().comic_op_lstm_gates_fwd(P(g), ptr(d_c), ptr(d_h), ptr(ex['ga']), ptr(ex['c_new']), ptr(ex['y']), ptr(d_mask),
                                          KEEP_OUT, ptr(d_lens), t, ptr(ex['cs']), ptr(ex['hs']), B, D, ptr(xh, xh_off), xh_ld, S,
                                          P(bias), stream()), 'lstm_gates_fwd_ex')
    L.check(lib().comic_lstm_gates_fwd(P(g32), ptr(d_c), ptr(d_h), ptr(pub['ga']), ptr(pub['c_new']), ptr(h_new),
                                       ptr(pub['y']), ptr(d_mask), KEEP_OUT, ptr(d_lens), t, ptr(pub['cs']), ptr(pub['hs']), B, D,
                                       stream()), 'lstm_gates_fwd')
    sync()
    for k in ex:
        chk('fwd %s vs the public op' % k, ex[k], host(pub[k]), 1e-6)
    # ... and both are the oracle's cell on the float64 sum of the operands
    gs = R.f64(g).sum(0) + bias
    i, j, f_, o = (gs[:, k * D:(k + 1) * D] for k in range(4))
    si, tj, sf, so = dr.sigmoid(i), np.tanh(j), dr.sigmoid(f_ + 1), dr.sigmoid(o)
    c2 = c * sf + si * tj
    h2 = np.tanh(c2) * so
    chk('fwd gates', ex['ga'], np.concatenate([si, tj, sf, so], 1), R.GATES_TOL, e)
    chk('fwd c_new', ex['c_new'], c2, R.GATES_TOL, e)
    chk('fwd y', ex['y'], dr.dropout(h2, R.f64(mask), KEEP_OUT), R.GATES_TOL, e)
    chk('fwd c_state', ex['cs'], np.where(fin[:, None], c, c2), R.GATES_TOL, e)
    hs_ref = np.where(fin[:, None], h, h2)
    chk('fwd h_state', ex['hs'], hs_ref, R.GATES_TOL, e)
    xh_h = host(xh)
    chk('fwd xh_next', xh_h[:, xh_off:xh_off + D], hs_ref, R.GATES_TOL, e)
    assert np.isnan(xh_h[:, :xh_off]).all() and np.isnan(xh_h[:, xh_off + D:]).all()
    # ---- backward: dy + S partials ----
    dy = rng.standard_normal((B, D)).astype(np.float32)
    dyp = partials(rng, S, B, D)
    dc = rng.standard_normal((B, D)).astype(np.float32)
    dh = rng.standard_normal((B, D)).astype(np.float32)
    dy32 = ((dy + dyp[0]) + dyp[1]) + dyp[2]
    e_dc, e_dh, e_dg, p_dc, p_dh, p_dg = dev(dc), dev(dh), nan(B, 4 * D), dev(dc), dev(dh), nan(B, 4 * D)
    L.check(lib().comic_op_lstm_gates_bwd(ptr(pub['ga']), ptr(d_c), ptr(pub['c_new']), P(dy), P(dyp), S, ptr(d_mask),
                                          KEEP_OUT, ptr(d_lens), t, ptr(e_dc), ptr(e_dh), ptr(e_dg), B, D, stream()), 'gates_bwd_ex')
    L.check(lib().comic_lstm_gates_bwd(ptr(pub['ga']), ptr(d_c), ptr(pub['c_new']), P(dy32), ptr(d_mask), KEEP_OUT,
                                       ptr(d_lens), t, ptr(p_dc), ptr(p_dh), ptr(p_dg), B, D, stream()), 'gates_bwd')
    sync()
    chk('bwd dg vs the public op', e_dg, host(p_dg), 1e-6)
    chk('bwd dc vs the public op', e_dc, host(p_dc), 1e-6)
    chk('bwd dh vs the public op', e_dh, host(p_dh), 1e-6)
    ga = R.f64(host(pub['ga']))
    live = (~fin)[:, None].astype(np.float64)
    dh2 = R.f64(dh) * live + dr.dropout(R.f64(dy) + R.f64(dyp).sum(0), R.f64(mask), KEEP_OUT)
    gates = tuple(ga[:, k * D:(k + 1) * D] for k in range(4)) + (np.tanh(R.f64(host(pub['c_new']))),)
    dg_ref, dcp_ref = dr._lstm_backward(None, gates, R.f64(c), R.f64(dc) * live, dh2, D)
    chk('bwd dg', e_dg, dg_ref, F32_RTOL)
    chk('bwd dc', e_dc, R.f64(dc) * (1 - live) + dcp_ref, F32_RTOL)


# ============================================================================ column sums ===========================
@pytest.mark.parametrize('cols', [1, 258, 1537])
@pytest.mark.parametrize('rows', [255, 256, 257, 1000])
def test_colsum_forms(rows, cols):
    """comic_colsum_ws takes its two-stage form from 256 rows on (with a workspace); comic_colsum is the one-stage form"""
    rng = np.random.default_rng(rows + cols)
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    pre = rng.standard_normal(cols).astype(np.float32)
    ref = R.f64(x).sum(0)
    d_x = dev(x)
    for beta in (0.0, 1.0):
        for form in ('ws', 'null ws', 'colsum'):
            out = nan(cols) if beta == 0.0 else dev(pre)
            ws = nan(64 * cols) if form == 'ws' else None
            if form == 'colsum':
                L.check(lib().comic_colsum(ptr(d_x), ptr(out), rows, cols, beta, stream()))
            else:
                L.check(lib().comic_op_colsum_ws(ptr(d_x), ptr(out), rows, cols, beta, ptr(ws), stream()))
            sync()
            chk('%s beta %g' % (form, beta), out, ref + beta * R.f64(pre), R.SUM_TOL)


# ============================================================================ split-K products =======================
GEMM_CASES = [(6, 512, 384, 0), (64, 2048, 2816, 0), (64, 512, 512, 0), (23, 2816, 2048, 1), (6, 384, 512, 1),
              (37, 258, 130, 0)]            # K = 130: no multiple of 16, too short to split


def expected_slices(M, N, K, ws_bytes):
    """comic_gemm_f32_partial's slice count, restated from csrc/gemm.hip"""
    KB, NB, MB = (K + 15) // 16, (N + 63) // 64, (M + 63) // 64
    S = max(1, min(256 // max(1, NB * MB), KB // 8, 32))
    while S > 1 and S * M * N * 4 > ws_bytes:
        S -= 1
    per = (KB + S - 1) // S
    return (KB + per - 1) // per


def gemm_operands(M, N, K, tb):
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    Bm = rng.standard_normal((N, K) if tb else (K, N)).astype(np.float32)
    return rng, A, Bm, R.f64(A) @ (R.f64(Bm).T if tb else R.f64(Bm))


@pytest.mark.parametrize('small_ws', [False, True])
@pytest.mark.parametrize('M,N,K,tb', GEMM_CASES)
def test_gemm_f32_partial(M, N, K, tb, small_ws):
    """the raw split-K slices the consumer kernels add up; a small workspace forces fewer slices"""
    rng, A, Bm, ref = gemm_operands(M, N, K, tb)
    full = expected_slices(M, N, K, 32 * M * N * 4)
    ws_floats = (max(1, full // 2) if small_ws else 32) * M * N
    want = expected_slices(M, N, K, ws_floats * 4)
    assert want <= full and (not small_ws or full == 1 or want < full)
    ws = nan(ws_floats)
    S = C.c_int(-1)
    L.check(lib().comic_gemm_f32_partial(P(A), P(Bm), M, N, K, K, Bm.shape[1], tb, ptr(ws), ws_floats * 4,
                                         C.byref(S), stream()), 'gemm_partial')
    sync()
    print('  slices %d (unconstrained %d)' % (S.value, full))
    assert S.value == want
    parts = host(ws)[:S.value * M * N].reshape(S.value, M, N)
    chk('sum of %d slices' % S.value, R.f64(parts).sum(0), ref, R.SUM_TOL)
    assert np.isnan(host(ws)[S.value * M * N:]).all(), 'written past the slices'


@pytest.mark.parametrize('M,N,K,tb', GEMM_CASES)
def test_gemm_f32_splitk(M, N, K, tb):
    """comic_gemm_f32_splitk: the checks of test_gemm_f32 (bias, alpha, beta, strided C) with a split-K workspace"""
    rng, A, Bm, ref = gemm_operands(M, N, K, tb)
    bias = rng.standard_normal(N).astype(np.float32)
    C0 = rng.standard_normal((M, N)).astype(np.float32)
    ws_floats = 32 * M * N
    ws = nan(ws_floats)
    dA, dB, dC = dev(A), dev(Bm), dev(C0)
    L.check(lib().comic_gemm_f32_splitk(ptr(dA), ptr(dB), ptr(dC), P(bias), M, N, K, K, Bm.shape[1], N, 0, tb, 0.5, 2.0,
                                        ptr(ws), ws_floats * 4, stream()))
    sync()
    chk('splitk alpha beta bias', dC, 0.5 * ref + 2.0 * R.f64(C0) + bias, R.SUM_TOL)
    big = nan(M, N + 8)
    L.check(lib().comic_gemm_f32_splitk(ptr(dA), ptr(dB), ptr(big), None, M, N, K, K, Bm.shape[1], N + 8, 0, tb, 1.0, 0.0,
                                        ptr(ws), ws_floats * 4, stream()))
    sync()
    chk('splitk strided C', host(big)[:, :N], ref, R.SUM_TOL)
    assert np.isnan(host(big)[:, N:]).all(), 'written outside the N columns of a strided C'
