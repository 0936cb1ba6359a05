"""Beam search with required words on the GPU: the bookkeeping operator (comic_beam_required_table) against
tests/beam_required_ref.base_and_specials, the banked step (comic_beam_step_required) against the float64 reference
ref_select_banks, its degenerate cases against the plain ensemble step, and the whole decoder (Decoder / EnsembleDecoder
.beam_search(required=)) against the reference loop.

Ids are compared exactly under the rule of tests/test_gpu_ensemble.py, applied per bank: every case asserts that its float64
reference separates the ranks 1 ... min(Wb, eligible) + 1 of every bank's eligible list by more than the bar (margin > 1) in
EVERY entry and EVERY bank; no entry is excused.  The margins quoted below were computed on the CPU with this reference."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import comic_amd._lib as L
from comic_amd import decoder as cdec
from comic_amd.decoder import BeamConstraints, BeamGroups, BeamRequired, BeamSampling
from tests import beam_constraints_ref as bref
from tests import beam_required_ref as rref
from tests.gpu_util import DEV, F32_RTOL, assert_close, dev, stream, sync
from tests.test_gpu_ensemble import POISON, _features, _rand_params, _spec_and_cfg, run_step

MAX_STEPS = 14


# ------------------------------------------------------------------ the bookkeeping operator ----------------------------
def _req_struct(C_, S):
    q = L.BeamRequired()
    q.n_words, q.stride = C_, S
    return q


# (B, W, V, C, S): smallest; two words; radix S = 2; more than 32 entries
TABLE_CASES = [(2, 4, 17, 1, 1), (3, 6, 258, 2, 1), (2, 10, 258, 2, 2), (33, 2, 258, 1, 1)]


@pytest.mark.parametrize('B,W,V,C_,S', TABLE_CASES)
def test_bookkeeping_matches_the_rule_step_by_step(B, W, V, C_, S):
    """Five consecutive steps from step 0 (null words / parents), both history buffers in play, random parents and words
    that are required tokens half of the time (so words complete, partials form and are lost); row 0's parents and words
    are hand-built: it follows itself and spells entry 0's first word, then repeats it."""
    lib = L.load()
    rng = np.random.default_rng(3)
    steps, max_steps = 5, 7
    req = rref.random_req(rng, B, C_, S, V, pad_last=True)
    d_req = dev(req)
    R = B * W
    hist = torch.full((2, R, max_steps), -7, dtype=torch.int32, device=DEV)
    base = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    special = torch.full((R, 4, 2), -7, dtype=torch.int32, device=DEV)
    q = _req_struct(C_, S)
    hists = [[] for _ in range(R)]
    words = parents = None
    for t in range(steps):
        if t > 0:
            parents = rng.integers(0, W, (B, W)).astype(np.int32)
            pick = req[np.arange(B)[:, None], rng.integers(0, C_, (B, W)), (t - 1) % S]
            words = np.where((rng.random((B, W)) < 0.5) & (pick >= 0), pick, rng.integers(0, V, (B, W))).astype(np.int32)
            parents[0, 0], words[0, 0] = 0, req[0, 0, (t - 1) % S]
            hists = [hists[(r // W) * W + int(parents.reshape(-1)[r])] + [int(words.reshape(-1)[r])] for r in range(R)]
        d_w, d_p = (dev(words), dev(parents)) if t > 0 else (None, None)
        L.check(lib.comic_beam_required_table(L.ptr(d_w), L.ptr(d_p), d_req.data_ptr(), hist.data_ptr(), base.data_ptr(),
                                              special.data_ptr(), C.byref(q), t, B, W, V, max_steps, V - 1, stream()),
                'beam_required_table')
        sync()
        ref_base, ref_special = rref.table_of(hists, req, S, W)
        np.testing.assert_array_equal(base.cpu().numpy().reshape(B, W), ref_base, err_msg='base at step %d' % t)
        np.testing.assert_array_equal(special.cpu().numpy().reshape(B, W, 4, 2), ref_special, err_msg='special at step %d' % t)
        got_hist = hist[t & 1].cpu().numpy()
        for r in range(R):
            assert got_hist[r, :t].tolist() == hists[r] and (got_hist[r, t:] == -7).all(), (t, r)
        if t > 0:
            assert ref_base.max() > ref_base.min() or C_ * S == 1                 # rows differ in progress
    assert rref.progress(hists[0], req[0], S) >= S                               # the hand-built row has met a word


def test_initial_state_from_the_padding_rows():
    lib = L.load()
    B, W, C_, S, V = 3, 10, 2, 2, 258
    req = np.array([[[5, 6], [7, 8]], [[5, 6], [-1, -1]], [[-1, -1], [-1, -1]]], np.int32)
    lp = torch.zeros((B, W), dtype=torch.float32, device=DEV)
    fin = torch.zeros((B, W), dtype=torch.int32, device=DEV)
    ln = torch.full((B, W), 9, dtype=torch.int64, device=DEV)
    q = _req_struct(C_, S)
    L.check(lib.comic_beam_required_init(dev(req).data_ptr(), lp.data_ptr(), fin.data_ptr(), ln.data_ptr(), B, W, V, V - 1,
                                         C.byref(q), stream()), 'beam_required_init')
    sync()
    ref_lp, ref_fin, ref_len = rref.init_state(req, W, S)
    assert np.argmax(ref_fin == 0, axis=1).tolist() == [0, 4, 8]
    np.testing.assert_array_equal(lp.cpu().numpy(), ref_lp)
    np.testing.assert_array_equal(fin.cpu().numpy(), ref_fin)
    np.testing.assert_array_equal(ln.cpu().numpy(), ref_len)


# ------------------------------------------------------------------ the banked step -----------------------------------------
def run_step_required(logits, wts, log_probs, finished, lengths, end_id, lpw, base, special, banks, bits=None, workspace=True):
    lib = L.load()
    n, B, W, V = logits.shape
    d_lg, d_lp, d_fin, d_len = dev(logits), dev(log_probs), dev(finished), dev(lengths)
    d_base, d_special = dev(np.ascontiguousarray(base, np.int32)), dev(np.ascontiguousarray(special, np.int32))
    d_bits = dev(np.ascontiguousarray(bits).view(np.int32)) if bits is not None else None
    word = torch.full((B, W), -1, dtype=torch.int32, device=DEV)
    parent = torch.full((B, W), -1, dtype=torch.int32, device=DEV)
    scores = torch.zeros((B, W), dtype=torch.float32, device=DEV)
    nbytes = int(lib.comic_beam_step_required_workspace(n, B, W, V))
    assert nbytes > int(lib.comic_beam_step_ensemble_workspace(n, B, W, V)) > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ws_ptr, ws_bytes = (ws.data_ptr(), nbytes) if workspace else (None, 0)
    wt = (C.c_float * n)(*[float(w) for w in wts])
    L.check(lib.comic_beam_step_required(d_lg.data_ptr(), wt, n, d_lp.data_ptr(), d_fin.data_ptr(), d_len.data_ptr(),
                                         word.data_ptr(), parent.data_ptr(), scores.data_ptr(), B, W, V, end_id, float(lpw),
                                         L.ptr(d_bits), (V + 31) // 32, d_base.data_ptr(), d_special.data_ptr(), banks, ws_ptr,
                                         ws_bytes, stream()), 'beam_step_required')
    sync()
    return dict(word=word.cpu().numpy(), parent=parent.cpu().numpy(), scores=scores.cpu().numpy(),
                log_probs=d_lp.cpu().numpy(), finished=d_fin.cpu().numpy(), lengths=d_len.cpu().numpy(),
                split=int(lib.comic_beam_step_ensemble_path()))


def _state(c):
    return c['logits'], c['wts'], c['log_probs'], c['finished'], c['lengths'], c['end_id']


def _check_step(got, ref):
    for k in ('word', 'parent', 'finished', 'lengths'):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    dead = ~np.isfinite(ref['scores'])
    np.testing.assert_array_equal(np.isneginf(got['scores']), dead, err_msg='dead slots (scores)')
    np.testing.assert_array_equal(np.isneginf(got['log_probs']), dead, err_msg='dead slots (log_probs)')
    assert_close(np.where(dead, 0, got['scores']), np.where(dead, 0, ref['scores']), F32_RTOL, 'scores')
    assert_close(np.where(dead, 0, got['log_probs']), np.where(dead, 0, ref['log_probs']), F32_RTOL, 'new log_probs')


# ((n, B, W, V), C, S, seed): smallest; three members; radix S = 2 (five banks); the split form; nine beams in the split form
# (W * kper = 45 register slots do not hold every row); eighteen beams in two banks; more than 32 entries.  Minimum margin
# over init / mid, lpw 0 / 0.7 and the rule / random tables, computed on the CPU: 55, 32, 21, 24, 23, 2.9, 28.
CASES = [((1, 2, 4, 17), 1, 1, 0), ((3, 3, 6, 258), 2, 1, 0), ((1, 2, 10, 258), 2, 2, 0), ((2, 2, 6, 9001), 2, 1, 0),
         ((1, 2, 9, 9001), 2, 1, 0), ((2, 2, 18, 9001), 1, 1, 1), ((1, 33, 2, 258), 1, 1, 0)]
STEP_CASES = [(shape, C_, S, seed, state, lpw, table) for shape, C_, S, seed in CASES for state in ('init', 'mid')
              for lpw in (0.0, 0.7) for table in ('rule', 'random')]
# every base 0 and nine live beams: bank 0 scans 9 rows x 5 columns per thread, past the 40 register slots (margin 143)
STEP_CASES.append(((1, 2, 9, 9001), 2, 1, 0, 'mid', 0.0, 'low'))


@pytest.mark.parametrize('shape,C_,S,seed,state,lpw,table', STEP_CASES)
def test_banked_step_matches_float64(shape, C_, S, seed, state, lpw, table):
    c = rref.banks_case(shape, C_, S, state, lpw, seed, table)
    ref, banks = c['ref'], c['banks']
    print('reference rank-gap margin %.2f (must exceed 1); eligible per bank %s' % (ref['margin'], ref['eligible'].tolist()))
    assert ref['margin'] > 1.0, 'the seed of this case does not separate the ranks of the float64 reference'
    Wb = shape[2] // banks
    if state == 'init':          # the banks decide: a kernel that ignored dest would give the plain step's selection
        assert not (np.array_equal(ref['word'], c['plain']['word']) and np.array_equal(ref['parent'], c['plain']['parent']))
        assert (ref['eligible'] < Wb).any() == (not np.isfinite(ref['scores']).all())         # a short bank: dead slots
    if table == 'rule' and state == 'mid' and C_ > 1:
        assert (ref['eligible'][0, :S] == 0).all()            # entry 0 has a padding row: its first S banks are empty
    got = run_step_required(*_state(c), lpw, c['base'], c['special'], banks)
    # the split form runs exactly where the rule of the plain step says, on the entry-wide W * V
    assert got['split'] == (1 if (shape[3] == 9001 and lpw == 0.0) else 0)
    _check_step(got, ref)
    dead = ~np.isfinite(ref['scores'])
    assert (got['parent'][dead] == np.tile(np.arange(shape[2]), (shape[1], 1))[dead]).all()
    assert (got['word'][dead] == c['end_id']).all() and (got['finished'][dead] == 1).all()
    np.testing.assert_array_equal(got['lengths'][dead], c['lengths'][dead])


@pytest.mark.parametrize('shape,C_,S', [((3, 3, 6, 258), 2, 1), ((2, 2, 6, 9001), 2, 1)])
def test_no_workspace_is_the_one_workgroup_form_with_the_same_ids(shape, C_, S):
    for state in ('init', 'mid'):
        c = rref.banks_case(shape, C_, S, state, 0.0)
        a = run_step_required(*_state(c), 0.0, c['base'], c['special'], c['banks'])
        b = run_step_required(*_state(c), 0.0, c['base'], c['special'], c['banks'], workspace=False)
        assert b['split'] == 0 and a['split'] == (1 if shape[3] == 9001 else 0)
        _check_step(b, c['ref'])
        for k in ('word', 'parent', 'finished', 'lengths'):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ------------------------------------------------------------------ with bans ------------------------------------------
@functools.lru_cache(maxsize=None)
def banned_case(shape, C_, S, state):
    """Half of all candidates banned, and with them every candidate the unbanned banked reference selects."""
    c = rref.banks_case(shape, C_, S, state, 0.0)
    n, B, W, V = shape
    mask = np.random.default_rng(1).random((B, W, V)) < 0.5
    mask[np.arange(B)[:, None], c['ref']['parent'], c['ref']['word']] = True
    live = c['finished'] == 0
    lp = np.where(mask & live[:, :, None], -np.inf, c['lp'])
    return c, mask, rref.ref_select_banks(lp, c['log_probs'], c['finished'], c['lengths'], c['end_id'], 0.0, c['base'],
                                          c['special'], c['banks'])


@pytest.mark.parametrize('shape,C_,S,state', [((3, 3, 6, 258), 2, 1, 'mid'), ((2, 2, 6, 9001), 2, 1, 'init'),
                                              ((2, 2, 6, 9001), 2, 1, 'mid')])
def test_banked_step_under_a_ban_mask(shape, C_, S, state):
    """Checked on the CPU: margins 30.3, 92.5 and 2.58.  A banned special leaves its bank empty: a dead slot, not a banned
    candidate."""
    c, mask, ref = banned_case(shape, C_, S, state)
    print('reference rank-gap margin %.2f (must exceed 1)' % ref['margin'])
    assert ref['margin'] > 1.0
    assert not np.array_equal(ref['word'], c['ref']['word']), 'the mask does not change what the step selects'
    n, B, W, V = shape
    got = run_step_required(*_state(c), 0.0, c['base'], c['special'], c['banks'], bits=bref.pack_bits(mask.reshape(B * W, V)))
    assert got['split'] == (1 if V == 9001 else 0)
    _check_step(got, ref)
    bidx = np.arange(B)[:, None]
    live_parent = (c['finished'][bidx, got['parent']] == 0) & np.isfinite(got['scores'])
    assert live_parent.any()
    assert not (mask[bidx, got['parent'], got['word']] & live_parent).any(), 'a banned candidate of a live beam was selected'


@pytest.mark.parametrize('shape,C_,S', [((3, 3, 6, 258), 2, 1), ((2, 2, 6, 9001), 2, 1)])
def test_all_zero_mask_is_no_mask_to_the_bit(shape, C_, S):
    n, B, W, V = shape
    for state in ('init', 'mid'):
        c = rref.banks_inputs(shape, C_, S, state)
        none = run_step_required(*_state(c), 0.0, c['base'], c['special'], c['banks'])
        zero = run_step_required(*_state(c), 0.0, c['base'], c['special'], c['banks'],
                                 bits=np.zeros((B * W, (V + 31) // 32), np.uint32))
        for k in ('word', 'parent', 'finished', 'lengths', 'scores', 'log_probs', 'split'):
            np.testing.assert_array_equal(zero[k], none[k], err_msg=k)


# ------------------------------------------------------------------ the top bank alone -----------------------------------
@pytest.mark.parametrize('shape,C_,S', [((3, 3, 6, 258), 2, 1), ((2, 2, 6, 9001), 2, 1), ((2, 2, 18, 9001), 1, 1)])
def test_all_padding_top_bank_is_the_ensemble_step_of_its_width(shape, C_, S):
    """A table of padding rows only: every beam lives in the top bank, whose rows are comic_beam_step_ensemble at width Wb
    on the same logits rows; every other bank stays dead.  Checked on the CPU: the narrow references' margins are 185 / 505, 207 / 736 and 2.9 / 2.3 (init / mid)."""
    from tests.test_gpu_ensemble import ref_select, ref_step_lp
    n, B, W, V = shape
    banks = C_ * S + 1
    Wb, top = W // banks, (banks - 1) * (W // banks)
    req = np.full((B, C_, S), -1, np.int32)
    for state in ('init', 'mid'):
        c = dict(rref.banks_inputs(shape, C_, S, 'mid', 0))
        if state == 'init':
            c['log_probs'], c['finished'], c['lengths'] = rref.init_state(req, W, S)
        else:                                                  # the top bank mid-decode (its last slot finished), the rest dead
            c['log_probs'] = c['log_probs'].copy()
            c['finished'] = np.ones((B, W), np.int32)
            c['log_probs'][:, :top] = -np.inf
            c['finished'][:, top:W - 1] = 0
        base, special = rref.table_of([[3, 4]] * (B * W), req, S, W)
        assert (base == banks - 1).all() and (special[..., 0] == -1).all()
        narrow_ref = ref_select(ref_step_lp(c['logits'][:, :, top:], c['wts']), c['log_probs'][:, top:], c['finished'][:, top:],
                                c['lengths'][:, top:], c['end_id'], 0.0)
        assert narrow_ref['margin'] > 1.0
        got = run_step_required(*_state(c), 0.0, base, special, banks)
        narrow = run_step(np.ascontiguousarray(c['logits'][:, :, top:]), c['wts'], c['log_probs'][:, top:].copy(),
                          c['finished'][:, top:].copy(), c['lengths'][:, top:].copy(), c['end_id'], 0.0)
        for k in ('word', 'finished', 'lengths'):
            np.testing.assert_array_equal(got[k][:, top:], narrow[k], err_msg=k)
        np.testing.assert_array_equal(got['parent'][:, top:], narrow['parent'] + top)
        assert_close(got['scores'][:, top:], narrow['scores'], F32_RTOL, 'scores')
        assert_close(got['log_probs'][:, top:], narrow['log_probs'], F32_RTOL, 'new log_probs')
        assert np.isneginf(got['scores'][:, :top]).all() and (got['finished'][:, :top] == 1).all()


# ------------------------------------------------------------------ refusals -------------------------------------------
def test_library_refuses_bad_banks_and_structs():
    lib = L.load()
    B, W, V = 1, 6, 17
    buf = torch.zeros(4096, dtype=torch.int32, device=DEV)
    wt = (C.c_float * 1)(1.0)
    p = buf.data_ptr()

    def step(banks, W=W):
        return lib.comic_beam_step_required(p, wt, 1, p, p, p, p, p, p, B, W, V, V - 1, 0.0, None, 0, p, p, banks, None, 0,
                                            stream())

    def table(q, W=W, V=V):
        return lib.comic_beam_required_table(None, None, p, p, p, p, C.byref(q) if q is not None else None, 0, B, W, V, 4,
                                             V - 1, stream())
    for call, what in ((lambda: step(4), 'banks 4 does not divide'), (lambda: step(1), 'banks must be in [2,17]'),
                       (lambda: step(18), 'banks must be'), (lambda: table(None), 'null required'),
                       (lambda: table(_req_struct(0, 1)), 'required.n_words'), (lambda: table(_req_struct(5, 1)), 'required.n_words'),
                       (lambda: table(_req_struct(1, 0)), 'required.stride'), (lambda: table(_req_struct(1, 5)), 'required.stride'),
                       (lambda: table(_req_struct(3, 1)), '4 banks'),
                       (lambda: table(_req_struct(1, 1), V=70000), 'exceeds 65536')):
        rc = call()
        assert rc != 0
        assert what in lib.comic_last_error().decode(), (what, lib.comic_last_error())
    sync()


def test_library_refuses_groups_and_sampling():
    """comic_decoder_beam_required checks them before it reads anything else."""
    lib = L.load()
    q, grp, smp = _req_struct(1, 1), L.BeamGroups(2, 0.5), L.BeamSampling()
    p = torch.zeros(64, dtype=torch.int32, device=DEV).data_ptr()

    def call(g, s):
        return lib.comic_decoder_beam_required(None, None, None, None, None, 1, 1, 2, 4, None, g, s, C.byref(q), p, None, None,
                                               None, None, None, None, None, None, 0, stream())
    assert call(C.byref(grp), None) != 0 and 'groups = 2 does not combine' in lib.comic_last_error().decode()
    assert call(None, C.byref(smp)) != 0 and 'sampling does not combine' in lib.comic_last_error().decode()


# ------------------------------------------------------------------ the whole decoder ------------------------------------
def _caption(res, b, slot):
    return res['predicted_ids'][:, b, slot].tolist()


def _trace(ref, b, slot):
    out, w = [], int(slot)
    for t in range(ref['step_ids'].shape[0] - 1, -1, -1):
        out.append(int(ref['step_ids'][t, b, w]))
        w = int(ref['parent_ids'][t, b, w])
    return out[::-1]


def _check_decode(res, ref, req, S, plain):
    assert res['step_ids'].shape[0] == ref['step_ids'].shape[0]                # steps_executed
    np.testing.assert_array_equal(res['step_ids'], ref['step_ids'])
    np.testing.assert_array_equal(res['parent_ids'], ref['parent_ids'])
    np.testing.assert_array_equal(res['lengths'], ref['lengths'])
    fin = np.isfinite(ref['scores'])
    np.testing.assert_array_equal(np.isfinite(res['scores']), fin)
    assert_close(np.where(fin, res['scores'], 0), np.where(fin, ref['scores'], 0), F32_RTOL, 'scores')
    assert_close(np.where(fin[-1], res['log_probs'], 0), np.where(fin[-1], ref['log_probs'], 0), F32_RTOL, 'final log_probs')
    banks = req.shape[1] * S + 1
    assert res['banks'] == banks == ref['banks']
    best, met = rref.result_rule(res['scores'][-1], banks, S)
    np.testing.assert_array_equal(res['best_slot'], best)
    np.testing.assert_array_equal(res['met'], met)
    np.testing.assert_array_equal(res['best_slot'], ref['best_slot'])
    Wb = res['scores'].shape[2] // banks
    full = 0
    for b in range(req.shape[0]):
        cap = _caption(res, b, int(res['best_slot'][b]))
        words = [row.tolist() for row in req[b] if row[0] >= 0]
        assert rref.progress(ref['hists'][b * res['scores'].shape[2] + int(best[b])], req[b], S) == best[b] // Wb
        if best[b] // Wb == banks - 1:                                           # the top bank: every word is in the caption
            full += 1
            for wd in words:
                assert any(cap[i:i + S] == wd for i in range(0, len(cap) - S + 1, S)), (b, wd, cap)
        mine = _trace(plain, b, 0)
        assert not all(any(mine[i:i + S] == wd for i in range(0, len(mine) - S + 1, S)) for wd in words), \
            'the decode without required words already contains them: the case shows nothing'
    assert full > 0, 'no image reaches its top bank: the case shows nothing'


@functools.lru_cache(maxsize=None)
def decode_case(name):
    """(members [(spec, cfg, params)], weights, W, S, req, cons, ref, plain) of a named decoder case; the required tokens are
    drawn (seeded) from those the unconstrained caption of the image does not hold; the last word of image 0 is padding."""
    geos, wts, W, C_, S, seed, eos, cons = dict(
        single=([{}], [1.0], 6, 2, 1, 61, 3.0, {}),
        radix=([{}], [1.0], 10, 2, 2, RADIX_SEED, 3.0, {}),
        two=([{}, dict(H=4)], [0.6, 0.4], 6, 2, 1, TWO_SEED, 3.0, {}),
        cons=([{}], [1.0], 6, 2, 1, CONS_SEED, 3.0, dict(min_length=6, no_repeat_ngram=2)),
        early=([{}], [1.0], 6, 2, 1, EARLY_SEED, 5.0, {}))[name]
    fm, im = _features()
    members = []
    for k, geo in enumerate(geos):
        spec, cfg = _spec_and_cfg(**geo)
        members.append((spec, cfg, _rand_params(cfg, seed + k, eos)))
    pc = [(p, cfg) for _, cfg, p in members]
    w32 = np.asarray(wts, np.float32)
    plain = bref.constrained_reference(pc, w32, fm, im, W, MAX_STEPS, **cons)
    req = _draw_req(plain, C_, S, members[0][0].V, 0)
    ref = rref.required_reference(pc, w32, fm, im, W, MAX_STEPS, req, S, **cons)
    return members, wts, W, S, req, cons, ref, plain


def _draw_req(plain, C_, S, V, tabseed):
    rng = np.random.default_rng(tabseed)
    B = plain['step_ids'].shape[1]
    req = np.full((B, C_, S), -1, np.int32)
    for b in range(B):
        cap = set(_trace(plain, b, 0))
        pool = [v for v in range(V - 1) if v not in cap]
        req[b] = rng.choice(pool, C_ * S, replace=False).reshape(C_, S)
    if C_ > 1:
        req[0, C_ - 1, :] = -1
    return req


RADIX_SEED, TWO_SEED, CONS_SEED, EARLY_SEED = 61, 47, 75, 53      # margins 27.7, 6.48, 2.19, 78.5 (3 steps)


def test_single_decoder_two_words():
    """C = 2, S = 1, W = 6.  Checked on the CPU: 14 steps, finished and live beams side by side, margin 6.41; every image
    reaches its top bank.  Eager, captured and replayed are equal to the bit with one context and one graph; a replay with a
    DIFFERENT table (other words, drawn alike) matches that table's reference through the same graph."""
    members, wts, W, S, req, cons, ref, plain = decode_case('single')
    spec, cfg, p = members[0]
    fm, im = _features()
    print('reference rank-gap margin over %d steps: %.2f (must exceed 1)' % (ref['step_ids'].shape[0], ref['margin']))
    assert ref['margin'] > 1.0 and ref['step_ids'].shape[0] == MAX_STEPS
    assert len(set(ref['lengths'].reshape(-1).tolist())) > 1
    dec = cdec.Decoder(spec, p, DEV)
    rq = BeamRequired(req)
    eager = dec.beam_search(dev(fm), dev(im), W, MAX_STEPS, want_attention=True, use_graph=False, required=rq)
    _check_decode(eager, ref, req, S, plain)
    dec.beam_search(dev(fm), dev(im), W, MAX_STEPS, required=rq)                  # captures
    replay = dec.beam_search(dev(fm), dev(im), W, MAX_STEPS, want_attention=True, required=BeamRequired(req.copy()))
    ctxs = dec._self_ensemble._ctxs
    assert len(ctxs) == 1 and next(iter(ctxs.values())).graph is not None
    for k in ('step_ids', 'parent_ids', 'predicted_ids', 'lengths', 'scores', 'log_probs', 'attn_hist', 'best_slot', 'met'):
        np.testing.assert_array_equal(replay[k], eager[k], err_msg='replay: ' + k)
    # another table through the same context and graph
    req2 = _draw_req(plain, req.shape[1], S, spec.V, 2)                        # checked on the CPU: margin 27.7
    ref2 = rref.required_reference([(p, cfg)], np.ones(1, np.float32), fm, im, W, MAX_STEPS, req2, S)
    print('second table: rank-gap margin %.2f' % ref2['margin'])
    assert ref2['margin'] > 1.0 and not np.array_equal(ref2['step_ids'], ref['step_ids'])
    other = dec.beam_search(dev(fm), dev(im), W, MAX_STEPS, want_attention=False, required=BeamRequired(req2))
    assert len(ctxs) == 1
    np.testing.assert_array_equal(other['step_ids'], ref2['step_ids'])
    np.testing.assert_array_equal(other['parent_ids'], ref2['parent_ids'])
    np.testing.assert_array_equal(other['best_slot'], ref2['best_slot'])
    np.testing.assert_array_equal(other['met'], ref2['met'])


@pytest.mark.parametrize('name', ['radix', 'two', 'cons'])
def test_decoder_cases(name):
    """radix: S = 2, W = 10 (five banks); two: members with different head counts, weights [0.6, 0.4]; cons: with
    BeamConstraints(min_length=6, no_repeat_ngram=2), the histories kept once.  Checked on the CPU: margins 27.7, 6.48 and 2.19, 14 steps each."""
    members, wts, W, S, req, cons, ref, plain = decode_case(name)
    fm, im = _features()
    print('reference rank-gap margin over %d steps: %.2f (must exceed 1)' % (ref['step_ids'].shape[0], ref['margin']))
    assert ref['margin'] > 1.0
    decs = [cdec.Decoder(spec, p, DEV) for spec, _, p in members]
    kw = dict(constraints=BeamConstraints(**cons)) if cons else {}
    if len(decs) == 1:
        res = decs[0].beam_search(dev(fm), dev(im), W, MAX_STEPS, want_attention=False, required=BeamRequired(req), **kw)
    else:
        res = cdec.EnsembleDecoder(decs, wts).beam_search(dev(fm), dev(im), W, MAX_STEPS, required=BeamRequired(req), **kw)
    _check_decode(res, ref, req, S, plain)


def test_early_exit_keeps_the_poison():
    """With the strong EOS bias the reference ends before max_steps.  Rows past steps_executed are never written, eager,
    captured or replayed."""
    members, wts, W, S, req, cons, ref, plain = decode_case('early')
    spec, cfg, p = members[0]
    fm, im = _features()
    T = ref['step_ids'].shape[0]
    print('reference: %d steps, rank-gap margin %.2f' % (T, ref['margin']))
    assert ref['margin'] > 1.0 and T < MAX_STEPS
    dec = cdec.Decoder(spec, p, DEV)
    for _ in range(3):
        res = dec.beam_search(dev(fm), dev(im), W, MAX_STEPS, want_attention=False, required=BeamRequired(req))
        _check_decode(res, ref, req, S, plain)
        ctx = next(iter(dec._self_ensemble._ctxs.values()))
        assert bool((ctx.step_ids[T:] == POISON).all()) and bool((ctx.parent_ids[T:] == POISON).all())
    assert ctx.graph is not None


def test_refused_on_the_host():
    spec, cfg = _spec_and_cfg()
    dec = cdec.Decoder(spec, _rand_params(cfg, 61, 3.0), DEV)
    fm, im = _features()
    ok = np.array([[[5], [6]]] * 3, np.int32)
    for req, kw, W, what in ((ok, {}, 4, '3 banks'), (np.zeros((3, 5, 1), np.int32), {}, 6, 'n_words must be'),
                             (np.zeros((3, 1, 5), np.int32), {}, 6, 'stride must be'),
                             (np.array([[[5], [spec.end_id]]] * 3), {}, 6, 'end_id'),
                             (np.array([[[5], [spec.V]]] * 3), {}, 6, 'outside the vocabulary'),
                             (ok[:2], {}, 6, 'the table holds 2 images'),
                             (ok, dict(groups=BeamGroups(2, 0.5)), 6, 'beam groups'),
                             (ok, dict(sampling=BeamSampling(1.0, 0)), 6, 'sampling')):
        with pytest.raises(ValueError, match=what):
            dec.beam_search(dev(fm), dev(im), W, MAX_STEPS, required=BeamRequired(req), **kw)
    assert '_self_ensemble' not in dec.__dict__                               # refused before anything was built


def test_none_changes_nothing():
    spec, cfg = _spec_and_cfg()
    p = _rand_params(cfg, 5, 3.0)
    fm, im = _features()
    dec = cdec.Decoder(spec, p, DEV)
    ens = cdec.EnsembleDecoder([dec, dec])
    for run, kw in ((dec.beam_search, dict(want_attention=False)), (ens.beam_search, dict())):
        base = run(dev(fm), dev(im), 6, MAX_STEPS, use_graph=False, **kw)
        assert not {'banks', 'best_slot', 'met', 'log_probs'} & set(base)
        res = run(dev(fm), dev(im), 6, MAX_STEPS, use_graph=False, required=None, **kw)
        assert sorted(res) == sorted(base)
        for k in base:
            np.testing.assert_array_equal(res[k], base[k], err_msg=k)
    plain_key = cdec.BeamOptions().ctx_key()                                      # the plain contexts only
    assert '_self_ensemble' not in dec.__dict__ and all(k[3] == plain_key for k in ens._ctxs)


# ------------------------------------------------------------------ CLI ---------------------------------------------------
from tests.test_gpu_constraints import tiny_run  # noqa: E402,F401  (the fixture: a one-epoch run on the tiny dataset)
from tests.test_gpu_ensemble import _run  # noqa: E402


def test_infer_cli_require_file(tiny_run, tmp_path):  # noqa: F811
    """--infer_require_file on the tiny dataset (radix tokens, one token per word): a known and an unknown word for image
    1 (by image_id), a known word for image 2 (by file name), nothing for the others.  Two words per image -> three banks
    at beam 6."""
    import json
    import os
    ds, run_dir, ckpt = tiny_run
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    num = os.path.basename(ckpt)[len('model_compact-'):-len('.npz')]
    tags = tmp_path / 'tags.json'
    tags.write_text(json.dumps({'1': ['frisbee', 'zebra'], 'COCO_test2014_000000000002.jpg': ['bench', 'train']}))
    common = ['--infer_checkpoints_dir', run_dir, '--dataset_dir', ds, '--infer_set', 'test', '--batch_size_infer', '2',
              '--get_metric_score', '', '--infer_checkpoints', num, '--infer_require_file', str(tags)]
    infer = os.path.join(root, 'src', 'infer.py')
    import subprocess
    import sys
    bad = subprocess.run([sys.executable, infer] + common + ['--infer_beam_size', '4'], capture_output=True, text=True)
    assert bad.returncode != 0 and 'infer_beam_size 4 is no multiple of 3' in bad.stderr, bad.stderr[-2000:]
    assert not [d for d in os.listdir(run_dir) if '_req' in d]                   # refused before anything was written
    _run(infer, common + ['--infer_beam_size', '6'])
    req_dir = os.path.join(run_dir, 'infer_test_beam_6_lpen_0.0_req2_tags')
    assert not os.path.exists(os.path.join(run_dir, 'infer_test_beam_6_lpen_0.0'))
    caps = json.load(open(os.path.join(req_dir, 'captions___%s.json' % num)))
    rows = json.load(open(os.path.join(req_dir, 'caption_required___%s.json' % num)))
    assert [r['image_id'] for r in rows] == [c['image_id'] for c in caps] == [1, 2, 3, 4]
    assert [r['required'] for r in rows] == [['frisbee'], ['bench', 'train'], [], []]
    assert [r['dropped'] for r in rows] == [['zebra'], [], [], []]
    for cap, r in zip(caps, rows):
        # a special always has a finite total here, so the top bank is reached: met counts the padding rows too
        assert r['met'] == 2 and r['bank'] == 2
        best = [x for x in r['captions'] if x['bank'] == r['bank']]
        assert len(best) == 1 and best[0]['caption'] == cap['caption'] and np.isfinite(best[0]['score'])
        assert [x['bank'] for x in r['captions']] == sorted(x['bank'] for x in r['captions'])
        for w in r['required']:
            assert w in cap['caption'].split(), (w, cap)
