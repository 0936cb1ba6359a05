"""Top-k / nucleus truncation of the sampled step on the GPU: the raw operator (comic_beam_truncate) against the float64
sandwich of tests/beam_truncate_ref.py, its composition with the sampled step, the whole decoder
(Decoder / EnsembleDecoder.beam_search(sampling=, truncation=)) and `infer.py`'s flags on the tiny dataset.

The pass rule is that of tests/beam_truncate_ref.check_mask: in EVERY live row the device keeps all of must_keep and none of
must_drop, with top-k alone exactly min(top_k, |A|) tokens, and leaves finished rows and pre-set bits alone; every case
asserts that its band holds at most 8 tokens per row and that must_keep is not empty.  The bands of all cases below were
computed on the CPU with that reference: at most 7 tokens.  ONE combination of the issue's grid cannot meet the cap and is
left out: V = 65 536 at temperature 1.0 with top_p = 0.9 alone, where a boundary token carries 6e-6 of the mass and the
band of top_p * (1 +- 1e-4) therefore holds 21 tokens; the same shape runs top_p = 0.9 at temperature 0.7 (band 7) and every
other operator at both temperatures."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import comic_amd._lib as L
from comic_amd import decoder as cdec
from comic_amd.decoder import BeamConstraints, BeamSampling, BeamTruncation
from oracle import decoder_ref as dr
from tests import beam_constraints_ref as bref
from tests import beam_sampling_ref as sref
from tests import beam_truncate_ref as tref
from tests.gpu_util import DEV, F32_RTOL, assert_close, dev, stream, sync
from tests.test_gpu_constraints import tiny_run  # noqa: F401  (the fixture: a one-epoch run on the tiny dataset)
from tests.test_gpu_ensemble import _features, _rand_params, _run, _spec_and_cfg
from tests.test_gpu_sampling import run_step_sampled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (n, B, W, V): smallest; radix vocabulary with three members; two members, more than one round per thread; the widest
# entry; V an exact multiple of 32 (the last mask word is full); the row that does not fit in LDS (scratch rows)
SHAPES = [(1, 2, 3, 17), (3, 3, 4, 258), (2, 2, 5, 9001), (1, 1, 64, 300), (1, 2, 2, 64), (1, 1, 2, 65536)]
OPS = [(1, 1.0), (5, 1.0), (40, 1.0), (0, 0.5), (0, 0.9), (5, 0.9)]          # (top_k, top_p)
CASES = [(s, state, temp) for s in SHAPES for state in ('init', 'mid') for temp in (0.7, 1.0)]
POISON_WORD = 0xA5A5A5A5


def _ops(shape, temp):
    return [(k, p) for k, p in OPS if k < shape[3] and not (shape[3] == 65536 and temp == 1.0 and (k, p) == (0, 0.9))]


def run_truncate(c, temp, top_k, top_p, banned=None):
    """-> the mask read back: dropped bool [B,W,V].  Without `banned` the incoming words are poison: the operator has to
    overwrite every one of them."""
    lib = L.load()
    n, B, W, V = c['logits'].shape
    words = (V + 31) // 32
    if banned is not None:
        bits = dev(np.ascontiguousarray(bref.pack_bits(banned.reshape(B * W, V))).view(np.int32))
    else:
        bits = torch.full((B * W, words), POISON_WORD - (1 << 32), dtype=torch.int32, device=DEV)
    nbytes = int(lib.comic_beam_truncate_workspace(n, B, W, V))
    assert nbytes >= 0
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
    wt = (C.c_float * n)(*[float(w) for w in c['wts']])
    trc = BeamTruncation(top_k, top_p).c_struct()
    d_lg, d_fin = dev(c['logits']), dev(c['finished'])
    L.check(lib.comic_beam_truncate(d_lg.data_ptr(), wt, n, d_fin.data_ptr(), bits.data_ptr(), words,
                                    B, W, V, float(temp), C.byref(trc), 0 if banned is None else 1,
                                    ws.data_ptr() if nbytes else None, nbytes, stream()), 'beam_truncate')
    sync()
    raw = bits.cpu().numpy().view(np.uint32)
    return tref.unpack_bits(raw, V).reshape(B, W, V), raw


@functools.lru_cache(maxsize=None)
def _ref(shape, state, temp, top_k, top_p, ban_seed=None):
    c = sref.sampled_inputs(shape, state)
    banned = _banned(shape, state, temp, ban_seed) if ban_seed is not None else None
    return tref.truncate_ref(c['lp'], c['finished'], sref.inv_temp_of(temp), top_k, top_p, banned)


# ------------------------------------------------------------------ 1. the raw operator against the sandwich -------------
@pytest.mark.parametrize('shape,state,temp', CASES)
def test_truncate_matches_the_sandwich(shape, state, temp):
    c = sref.sampled_inputs(shape, state)
    for top_k, top_p in _ops(shape, temp):
        ref = _ref(shape, state, temp, top_k, top_p)
        print('top_k %d top_p %g: band %d, smallest must_keep %d, k_clear %s' % (top_k, top_p, ref['band'], ref['keep_min'],
                                                                              ref['k_clear']))
        if top_p < 1.0 and top_k >= 1:
            assert ref['k_clear'], 'the nucleus of this case is not taken on an exact K'
        dropped, _ = run_truncate(c, temp, top_k, top_p)
        tref.check_mask(dropped, ref, top_k, top_p)
        if top_k == 1:                                          # exactly the reference argmax
            assert ref['k_clear']
            tref.check_mask(dropped, ref, top_k, top_p, exact=True)
            live = c['finished'] == 0
            np.testing.assert_array_equal(np.argmin(dropped, axis=2)[live], np.argmax(c['lp'], axis=2)[live])


def test_truncate_peaked_logits():
    """The regime `peaked` of tests/regimes.py on the widest entry (64 rows of V = 300), temperature 1: rows 30 N(0,1) + 200 /
    - 200 whose dominant token alone holds all but 1e-11 of the mass -- the first token exceeds p, the nucleus is that token
    -- and one row whose masses are 0.30, 0.25, 0.20, 0.14, 0.06 and a tail of 0.05: p = 0.9 is reached only at the fifth
    token (0.89 before it), p = 0.5 at the second (0.30 before it).  The pass rule is the sibling's."""
    shape = (1, 1, 64, 300)
    c = sref.peaked_inputs(shape)
    V, row = shape[3], int(np.flatnonzero(c['finished'][0] == 0)[3])
    q = np.r_[0.30, 0.25, 0.20, 0.14, 0.06, np.full(V - 5, 0.05 / (V - 5))]
    c['logits'][0, 0, row] = (200.0 + np.log(q))[np.random.default_rng(3).permutation(V)]
    c['lp'] = sref.ref_step_lp(c['logits'], c['wts'])
    for top_k, top_p in ((0, 0.9), (0, 0.5), (5, 0.9), (5, 1.0), (1, 1.0)):
        ref = tref.truncate_ref(c['lp'], c['finished'], sref.inv_temp_of(1.0), top_k, top_p)
        print('peaked top_k %d top_p %g: band %d, smallest must_keep %d, k_clear %s' % (top_k, top_p, ref['band'], ref['keep_min'],
                                                                                     ref['k_clear']))
        assert ref['k_clear']
        if top_p < 1.0:                                         # the reference itself: one token, and five / two in the crafted row
            kept = {bw: int(r['exact'].sum()) for bw, r in ref['rows'].items() if r is not None}
            # (within the top five, whose mass is 0.95, p = 0.9 is reached at the fourth token)
            assert kept[0, row] == {(0, 0.9): 5, (0, 0.5): 2, (5, 0.9): 4}[top_k, top_p]
            assert all(n == 1 for bw, n in kept.items() if bw != (0, row))
            assert ref['band'] == 0
        dropped, _ = run_truncate(c, 1.0, top_k, top_p)
        tref.check_mask(dropped, ref, top_k, top_p, exact=top_p < 1.0 or top_k == 1)


# ------------------------------------------------------------------ 2. under an incoming ban mask ------------------------
@functools.lru_cache(maxsize=None)
def _banned(shape, state, temp, ban_seed):
    """The float64 top 3 of every row and a random tenth of the vocabulary."""
    c = sref.sampled_inputs(shape, state)
    n, B, W, V = shape
    banned = np.random.default_rng(ban_seed).random((B, W, V)) < 0.1
    top3 = np.argsort(-c['lp'], axis=2, kind='stable')[:, :, :3]
    np.put_along_axis(banned, top3, True, axis=2)
    return banned


@pytest.mark.parametrize('shape', SHAPES)
def test_truncate_under_a_ban_mask(shape):
    """State mid, temperature 0.7.  The banned bits survive, k counts allowed tokens only, and the kept set is the sandwich of
    the allowed set.  Bands computed on the CPU: at most 7."""
    c = sref.sampled_inputs(shape, 'mid')
    banned = _banned(shape, 'mid', 0.7, 1)
    for top_k, top_p in ((5, 1.0), (0, 0.9), (5, 0.9)):
        ref = _ref(shape, 'mid', 0.7, top_k, top_p, 1)
        print('top_k %d top_p %g: band %d, k_clear %s' % (top_k, top_p, ref['band'], ref['k_clear']))
        assert ref['k_clear'] or top_p >= 1.0
        dropped, _ = run_truncate(c, 0.7, top_k, top_p, banned)
        tref.check_mask(dropped, ref, top_k, top_p, banned)
        live = c['finished'] == 0
        assert (dropped | ~banned).all(), 'a banned bit was cleared'
        if top_p >= 1.0:
            np.testing.assert_array_equal((~dropped).sum(axis=2)[live], 5)
        np.testing.assert_array_equal(dropped[~live], banned[~live])             # finished rows: as they came


# ------------------------------------------------------------------ 3. exact ties ------------------------------------------
@pytest.mark.parametrize('shape', [(1, 2, 3, 17), (1, 3, 4, 258), (1, 2, 5, 9001), (1, 1, 2, 65536)])
def test_exact_ties(shape):
    """One member, integer-valued logits in [-4, 4]: equal logits give equal lp bits on both sides and different ones are
    far apart, so the float64 rule's own set is asked for bit by bit: top-k keeps the lowest v among the tied, top-p keeps
    whole tie groups.  The reference's nucleus is the same at top_p * (1 +- GAP) (band 0), asserted."""
    n, B, W, V = shape
    rng = np.random.default_rng(3)
    c = dict(logits=rng.integers(-4, 5, (n, B, W, V)).astype(np.float32), wts=np.ones(1, np.float32),
             finished=np.zeros((B, W), np.int32))
    from tests.test_gpu_ensemble import ref_step_lp
    lp = ref_step_lp(c['logits'], c['wts'])
    tied_at_k = False
    for top_k, top_p in ((1, 1.0), (5, 1.0), (min(40, V - 1), 1.0), (0, 0.5), (0, 0.9)):
        ref = tref.truncate_ref(lp, c['finished'], sref.inv_temp_of(0.7), top_k, top_p)
        if top_p < 1.0:
            assert ref['band'] == 0
        dropped, _ = run_truncate(c, 0.7, top_k, top_p)
        for (b, w), r in ref['rows'].items():
            np.testing.assert_array_equal(~dropped[b, w], r['exact'], err_msg='top_k %d top_p %g row (%d, %d)' % (top_k, top_p, b, w))
            tied_at_k = tied_at_k or not r['k_clear']
    assert tied_at_k, 'no row of this case has a tie at its k-th value'


# ------------------------------------------------------------------ 4. no-ops ----------------------------------------------
@pytest.mark.parametrize('shape', [(3, 3, 4, 258), (1, 2, 2, 64), (1, 1, 2, 65536)])
def test_a_top_k_that_reaches_v_changes_nothing(shape):
    n, B, W, V = shape
    c = sref.sampled_inputs(shape, 'mid')
    for top_k in (V, V + 7):
        dropped, raw = run_truncate(c, 0.7, top_k, 1.0)
        assert not raw.any(), 'without bans the mask of a no-op is all zeros'
        banned = _banned(shape, 'mid', 0.7, 2)
        dropped, raw = run_truncate(c, 0.7, top_k, 1.0, banned)
        np.testing.assert_array_equal(raw, bref.pack_bits(banned.reshape(B * W, V)))


def test_finished_rows_are_untouched():
    shape = (2, 2, 5, 9001)
    n, B, W, V = shape
    c = dict(sref.sampled_inputs(shape, 'mid'))
    c['finished'] = np.ones((B, W), np.int32)
    banned = _banned(shape, 'mid', 0.7, 2)
    _, raw = run_truncate(c, 0.7, 5, 0.9, banned)
    np.testing.assert_array_equal(raw, bref.pack_bits(banned.reshape(B * W, V)))
    _, raw = run_truncate(c, 0.7, 5, 0.9)
    assert not raw.any()


# ------------------------------------------------------------------ 5. determinism -----------------------------------------
@pytest.mark.parametrize('shape,top_k,top_p', [((2, 2, 5, 9001), 0, 0.9), ((2, 2, 5, 9001), 40, 0.5), ((1, 1, 2, 65536), 5, 0.9),
                                               ((1, 1, 2, 65536), 0, 0.9)])
def test_two_runs_give_the_same_words(shape, top_k, top_p):
    c = sref.sampled_inputs(shape, 'mid')
    a = run_truncate(c, 0.7, top_k, top_p)[1]
    b = run_truncate(c, 0.7, top_k, top_p)[1]
    np.testing.assert_array_equal(a, b)
    assert a.any()


# ------------------------------------------------------------------ 6. composition with the sampled step -------------------
@pytest.mark.parametrize('shape,top_k,top_p', [((3, 3, 4, 258), 5, 0.9), ((2, 2, 5, 9001), 0, 0.9), ((2, 2, 5, 9001), 5, 1.0),
                                               ((1, 1, 64, 300), 5, 0.9)])
def test_the_sampled_step_under_the_device_mask(shape, top_k, top_p):
    """comic_beam_step_sampled under the mask comic_beam_truncate made equals the float64 sampled step with lp = -inf at that
    same mask read back, under the per-slot margin rule of tests/beam_sampling_ref.py, asserted.  Noise seed 5, base 0, t 0,
    state mid, temperature 0.7; margins computed on the CPU with the float64 rule's own mask, and with the band kept or
    dropped: 229 at the least."""
    n, B, W, V = shape
    c = sref.sampled_inputs(shape, 'mid')
    dropped, raw = run_truncate(c, 0.7, top_k, top_p)
    live = c['finished'] == 0
    lp = np.where(dropped & live[:, :, None], -np.inf, c['lp'])
    g = sref.noise(5, 0, B, W, 0, V)[2]
    ref = sref.ref_select_sampled(lp, c['log_probs'], c['finished'], c['lengths'], c['end_id'], g, sref.inv_temp_of(0.7))
    print('reference rank-gap margin %.2f (must exceed 1)' % ref['margin'])
    assert ref['margin'] > 1.0
    got = run_step_sampled(c['logits'], c['wts'], c['log_probs'], c['finished'], c['lengths'], c['end_id'], 0.7, bits=raw)
    for k in ('word', 'finished', 'lengths'):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert_close(got['log_probs'], ref['log_probs'], F32_RTOL, 'new log_probs')
    bidx = np.arange(B)[:, None]
    assert not (dropped[bidx, got['parent'], got['word']] & live).any(), 'a dropped candidate of a live slot was selected'
    # top-k decides: some live slot leaves the choice of the untruncated sampled step (2, 5 and 28 slots on the CPU)
    if top_k:
        plain = sref.sampled_case(shape, 'mid', 0.7)['ref']
        assert (plain['word'] != ref['word'])[live].any()


# ------------------------------------------------------------------ 7. the loop on the tiny model --------------------------
N_DEC, MAX_STEPS = 4, 14


def _members(two=False):
    out = []
    for seed, geo in ((61, dict()), (43, dict(H=4)))[:2 if two else 1]:
        spec, cfg = _spec_and_cfg(**geo)
        out.append((spec, cfg, _rand_params(cfg, seed, 3.0)))
    return out


def _forced_lp(members, wts, fm, im, W, step_ids):
    """The oracle's float64 step distributions lp [T,B,W,V], teacher-forced on the emitted ids [T,B,W] (a slot's parent is
    the slot itself, so no state is re-ordered)."""
    B = fm.shape[0]
    cfg0 = members[0][1]
    V = cfg0.softmax_size
    st = []
    for _, cfg, p in members:
        keys, values = dr.memory_projections(p, cfg, np.repeat(fm, W, axis=0))
        c, h, _ = dr.rnn_init(p, cfg, np.repeat(im, W, axis=0), None)
        st.append(dict(keys=keys, values=values, c=c, h=h, att=np.zeros((B * W, cfg.attn_size), np.float32)))
    ids = np.full(B * W, cfg0.start_id, np.int64)
    out = []
    from tests.test_gpu_ensemble import ref_step_lp
    for t in range(step_ids.shape[0]):
        logits = []
        for (_, cfg, p), s in zip(members, st):
            y, s['c'], s['h'], s['att'], _, _ = dr.decoder_step(p, cfg, s['keys'], s['values'], dr.embed(p['emb'], ids),
                                                                s['c'], s['h'], s['att'], None)
            logits.append((y @ p['W_o'] + p['b_o']).reshape(B, W, V))
        out.append(ref_step_lp(np.stack(logits), wts))
        ids = step_ids[t].reshape(-1).astype(np.int64)
    return np.stack(out)


def _check_top_k(res, members, wts, fm, im, temp, top_k, end_id):
    """Every token a live slot emitted is none of the oracle's must_drop at that step (the top-k band on top)."""
    ids = res['step_ids']
    T, B, W = ids.shape
    lp = _forced_lp(members, np.asarray(wts, np.float32), fm, im, W, ids)
    fin = np.zeros((B, W), bool)
    checked = 0
    for t in range(T):
        a = lp[t] * np.float64(sref.inv_temp_of(temp))
        for b in range(B):
            for w in range(W):
                if fin[b, w]:
                    continue
                r = tref.truncate_row(a[b, w], np.ones(a.shape[-1], bool), top_k, 1.0)
                assert not r['must_drop'][ids[t, b, w]], 'step %d slot (%d, %d) emitted %d, outside the top %d' % (
                    t, b, w, ids[t, b, w], top_k)
                checked += 1
        fin |= ids[t] == end_id
    assert checked > T


def _captions(res, spec):
    T, B, W = res['predicted_ids'].shape
    caps = np.full((B * W, T + 1), -1, np.int64)
    caps[:, 0] = spec.start_id
    ids = res['predicted_ids'].transpose(1, 2, 0).reshape(B * W, T)
    ln = res['lengths'].reshape(-1)
    for r in range(B * W):
        caps[r, 1:1 + ln[r]] = ids[r, :ln[r]]
    return caps


@pytest.mark.parametrize('temp', [0.7, 1.0])
def test_top_k_1_is_greedy_whatever_the_seed(temp):
    fm, im = _features()
    spec, cfg, p = _members()[0]
    dec = cdec.Decoder(spec, p, DEV)
    greedy = dec.beam_search(dev(fm), dev(im), 1, MAX_STEPS, want_attention=False)['predicted_ids'][:, :, 0]      # (T, B)
    for seed in (2, 3):
        res = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=False, sampling=BeamSampling(temp, seed),
                              truncation=BeamTruncation(top_k=1))
        T = min(greedy.shape[0], res['predicted_ids'].shape[0])
        assert T == greedy.shape[0]
        for w in range(N_DEC):
            np.testing.assert_array_equal(res['predicted_ids'][:T, :, w], greedy[:T], err_msg='seed %d slot %d' % (seed, w))


def test_single_decoder_top_k_3():
    """top_k = 3 at temperature 0.8: the emitted tokens against the oracle, log_probs against Decoder.score, the same seed the
    same bits (eager, capture, replay), another seed on the captured graph other captions, and a context of its own beside
    the untruncated one."""
    fm, im = _features()
    members = _members()
    spec, cfg, p = members[0]
    dec = cdec.Decoder(spec, p, DEV)
    smp, trc = BeamSampling(0.8, 2), BeamTruncation(top_k=3)
    eager = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=False, use_graph=False, sampling=smp, truncation=trc)
    _check_top_k(eager, members, [1.0], fm, im, 0.8, 3, spec.end_id)
    assert (eager['parent_ids'] == np.arange(N_DEC)).all()
    dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=False, sampling=smp, truncation=trc)      # captures
    replay = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=False, sampling=smp, truncation=trc)
    ctxs = dec._self_ensemble._ctxs
    assert len(ctxs) == 1 and next(iter(ctxs.values())).graph is not None
    for k in ('step_ids', 'parent_ids', 'predicted_ids', 'lengths', 'scores', 'log_probs'):
        np.testing.assert_array_equal(replay[k], eager[k], err_msg='replay: ' + k)
    other = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=False, sampling=BeamSampling(0.8, 3), truncation=trc)
    assert len(ctxs) == 1, 'a new seed must not build or capture anything'
    T = min(other['predicted_ids'].shape[0], eager['predicted_ids'].shape[0])
    assert not np.array_equal(other['predicted_ids'][:T], eager['predicted_ids'][:T])
    _check_top_k(other, members, [1.0], fm, im, 0.8, 3, spec.end_id)
    # the log-probabilities are the model's own, untruncated: Decoder.score of the captions reproduces them
    B = fm.shape[0]
    rep = lambda a: dev(np.repeat(a, N_DEC, axis=0))
    sc = dec.score(rep(fm), rep(im), _captions(eager, spec), use_graph=False)
    assert_close(sc['log_prob'].cpu().numpy().reshape(B, N_DEC), eager['log_probs'], F32_RTOL, 'Decoder.score of the samples')
    # untruncated sampling with the same seed is another context and other captions; an inactive truncation is that path
    plain = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=False, sampling=smp)
    same = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=False, sampling=smp, truncation=BeamTruncation())
    assert len(ctxs) == 2
    np.testing.assert_array_equal(plain['step_ids'], same['step_ids'])
    Tp = min(plain['predicted_ids'].shape[0], eager['predicted_ids'].shape[0])
    assert not np.array_equal(plain['predicted_ids'][:Tp], eager['predicted_ids'][:Tp])


def test_top_p_and_both_stages_run_the_loop():
    """top_p = 0.5 alone and (top_k = 3, top_p = 0.9): every emitted token is one of the oracle's top 3 where k is set, the
    log_probs are Decoder.score's, and the nucleus narrows the draw: its captions differ from the untruncated ones."""
    fm, im = _features()
    members = _members()
    spec, cfg, p = members[0]
    dec = cdec.Decoder(spec, p, DEV)
    smp = BeamSampling(1.0, 2)
    plain = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=False, sampling=smp)
    B = fm.shape[0]
    rep = lambda a: dev(np.repeat(a, N_DEC, axis=0))
    for trc in (BeamTruncation(top_p=0.5), BeamTruncation(3, 0.9)):
        res = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=False, sampling=smp, truncation=trc)
        if trc.top_k:
            _check_top_k(res, members, [1.0], fm, im, 1.0, 3, spec.end_id)
        sc = dec.score(rep(fm), rep(im), _captions(res, spec), use_graph=False)
        assert_close(sc['log_prob'].cpu().numpy().reshape(B, N_DEC), res['log_probs'], F32_RTOL, 'Decoder.score of the samples')
        T = min(plain['predicted_ids'].shape[0], res['predicted_ids'].shape[0])
        assert not np.array_equal(plain['predicted_ids'][:T], res['predicted_ids'][:T])


def test_the_same_captions_whatever_the_batching():
    a, b = _features(21), _features(22)
    fm, im = np.concatenate([a[0], b[0][:1]]), np.concatenate([a[1], b[1][:1]])
    spec, cfg, p = _members()[0]
    dec = cdec.Decoder(spec, p, DEV)
    smp, trc = BeamSampling(0.8, 2), BeamTruncation(3, 0.9)
    whole = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=False, sampling=smp, truncation=trc)
    for base in (0, 2):
        half = dec.beam_search(dev(fm[base:base + 2]), dev(im[base:base + 2]), N_DEC, MAX_STEPS, want_attention=False,
                               sampling=smp, image_base=base, truncation=trc)
        T = half['step_ids'].shape[0]
        np.testing.assert_array_equal(half['predicted_ids'], whole['predicted_ids'][:T, base:base + 2])
        assert (whole['predicted_ids'][T:, base:base + 2] == spec.end_id).all()
        np.testing.assert_array_equal(half['lengths'], whole['lengths'][base:base + 2])
        assert_close(half['log_probs'], whole['log_probs'][base:base + 2], F32_RTOL, 'log_probs of a half')


def test_truncation_with_constraints():
    """min_length 6 and no repeated bigram under (top_k = 3, top_p = 0.9): no banned token is emitted -- no <EOS> before
    step 6, no caption shorter than 6, no bigram twice in a caption."""
    fm, im = _features()
    spec, cfg, p = _members()[0]
    dec = cdec.Decoder(spec, p, DEV)
    res = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=False,
                          constraints=BeamConstraints(min_length=6, no_repeat_ngram=2), sampling=BeamSampling(0.8, 5),
                          truncation=BeamTruncation(3, 0.9))
    assert res['lengths'].min() >= 6
    assert not (res['step_ids'][:5] == spec.end_id).any()
    ids, ln = res['predicted_ids'], res['lengths']
    for b in range(ids.shape[1]):
        for w in range(N_DEC):
            cap = ids[:ln[b, w], b, w].tolist()
            grams = list(zip(cap, cap[1:]))
            assert len(grams) == len(set(grams)), 'a bigram repeats in %r' % (cap,)


def test_ensemble_of_two_members():
    fm, im = _features()
    members = _members(two=True)
    wts = [0.6, 0.4]
    ens = cdec.EnsembleDecoder([cdec.Decoder(spec, p, DEV) for spec, _, p in members], wts)
    smp, trc = BeamSampling(0.8, 3), BeamTruncation(top_k=3)
    res = ens.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, sampling=smp, truncation=trc)
    _check_top_k(res, members, wts, fm, im, 0.8, 3, members[0][0].end_id)
    again = ens.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, sampling=smp, truncation=trc)
    for k in ('step_ids', 'lengths', 'scores', 'log_probs'):
        np.testing.assert_array_equal(again[k], res[k], err_msg=k)
    one = ens.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, sampling=smp, truncation=BeamTruncation(top_k=1))
    greedy = ens.beam_search(dev(fm), dev(im), 1, MAX_STEPS)['predicted_ids'][:, :, 0]           # top_k = 1 is beam 1
    assert one['predicted_ids'].shape[0] == greedy.shape[0]
    for w in range(N_DEC):
        np.testing.assert_array_equal(one['predicted_ids'][:, :, w], greedy, err_msg='slot %d' % w)


# ------------------------------------------------------------------ 8. refusals --------------------------------------------
def test_refused_on_the_host_and_by_the_executor():
    spec, cfg, p = _members()[0]
    dec = cdec.Decoder(spec, p, DEV)
    fm, im = _features()
    smp = BeamSampling(0.8, 1)
    for kw, what in ((dict(truncation=BeamTruncation(5)), 'sampling'),
                     (dict(truncation=BeamTruncation(5), sampling=BeamSampling(0.8, 1, enabled=False)), 'sampling'),
                     (dict(truncation=BeamTruncation(-1), sampling=smp), 'top_k'),
                     (dict(truncation=BeamTruncation(0, 0.0), sampling=smp), 'top_p'),
                     (dict(truncation=BeamTruncation(0, float('nan')), sampling=smp), 'top_p')):
        with pytest.raises(ValueError, match=what):
            dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, **kw)
    assert '_self_ensemble' not in dec.__dict__                               # refused before anything was built
    lib = L.load()
    ens = cdec.EnsembleDecoder([dec])
    ctx = ens._ctx(fm.shape[0], N_DEC, MAX_STEPS, [(dev(fm), dev(im))],
                   cdec.BeamOptions(sampling=smp, truncation=BeamTruncation(5)))

    def call(s, t):
        return lib.comic_decoder_beam_truncated(ctx.descs, ctx.ptabs, ctx.fm_ptrs, ctx.im_ptrs, ctx.wts, 1, fm.shape[0], N_DEC,
                                                MAX_STEPS, None, s, t, ctx.step_ids.data_ptr(), ctx.parent_ids.data_ptr(),
                                                ctx.scores.data_ptr(), ctx.lengths.data_ptr(), ctx.finished.data_ptr(),
                                                ctx.hist_ptrs, ctx.steps.data_ptr(), ctx.ws.data_ptr(), ctx.nbytes, stream())
    s = C.byref(ctx.smp)
    V = spec.V
    for smp_arg, trc, what in ((None, L.BeamTruncation(5, 1.0), 'null sampling'), (s, None, 'null truncation'),
                               (s, L.BeamTruncation(-1, 1.0), 'top_k'), (s, L.BeamTruncation(5, 0.0), 'top_p'),
                               (s, L.BeamTruncation(5, -1.0), 'top_p'), (s, L.BeamTruncation(5, float('nan')), 'top_p'),
                               (s, L.BeamTruncation(0, 1.0), 'both stages'), (s, L.BeamTruncation(0, 2.0), 'both stages'),
                               (s, L.BeamTruncation(V, 1.0), 'does nothing'), (s, L.BeamTruncation(V + 3, 1.5), 'does nothing')):
        assert call(smp_arg, C.byref(trc) if trc is not None else None) != 0
        assert what in lib.comic_last_error().decode(), (what, lib.comic_last_error())
    # the raw operator: a vocabulary beyond 65 536, a wrong word count, a bad temperature
    buf = torch.zeros(8192, dtype=torch.int32, device=DEV)
    wt = (C.c_float * 1)(1.0)
    q = buf.data_ptr()
    trc = L.BeamTruncation(5, 0.9)
    for V_, words, temp, what in ((65537, 2049, 1.0, 'V = 65537'), (300, 9, 1.0, 'mask words'), (300, 10, 0.0, 'temperature')):
        assert lib.comic_beam_truncate(q, wt, 1, q, q, words, 1, 2, V_, temp, C.byref(trc), 0, None, 0, stream()) != 0
        assert what in lib.comic_last_error().decode(), (what, lib.comic_last_error())
    big = dev(sref.sampled_inputs((1, 1, 2, 65536), 'mid')['logits'])
    assert lib.comic_beam_truncate(big.data_ptr(), wt, 1, q, q, 2048, 1, 2, 65536, 1.0, C.byref(trc), 0, None, 0,
                                   stream()) != 0
    assert 'workspace too small' in lib.comic_last_error().decode()
    sync()


# ------------------------------------------------------------------ 9. CLI ----------------------------------------------------
def test_infer_cli_flags_write_both_files_in_a_directory_of_their_own(tiny_run):  # noqa: F811
    ds, run_dir, ckpt = tiny_run
    num = os.path.basename(ckpt)[len('model_compact-'):-len('.npz')]
    common = ['--infer_checkpoints_dir', run_dir, '--dataset_dir', ds, '--infer_set', 'test', '--batch_size_infer', '2',
              '--get_metric_score', '', '--infer_checkpoints', num, '--infer_beam_size', '4']
    sampled = common + ['--infer_sample', '--infer_temperature', '0.7', '--infer_sample_seed', '3']
    out_dir = os.path.join(run_dir, 'infer_test_beam_4_lpen_0.0_smp_t0.7_s3_k5_p0.9')
    _run(os.path.join(ROOT, 'src', 'infer.py'), sampled + ['--infer_top_k', '5', '--infer_top_p', '0.9'])
    caps = json.load(open(os.path.join(out_dir, 'captions___%s.json' % num)))
    samples = json.load(open(os.path.join(out_dir, 'caption_samples___%s.json' % num)))
    assert not os.path.exists(os.path.join(run_dir, 'infer_test_beam_4_lpen_0.0_smp_t0.7_s3'))
    assert len(caps) == 4 and len(samples) == 4
    for cap, s in zip(caps, samples):
        assert s['image_id'] == cap['image_id'] and [x['sample'] for x in s['captions']] == [0, 1, 2, 3]
        lps = [x['log_prob'] for x in s['captions']]
        assert all(np.isfinite(v) and v <= 0.0 for v in lps)
        assert s['captions'][int(np.argmax(lps))]['caption'] == cap['caption']
    with pytest.raises(ValueError, match='infer_sample'):
        _run(os.path.join(ROOT, 'src', 'infer.py'), common + ['--infer_top_k', '5'])
    with pytest.raises(ValueError, match='top_p'):
        _run(os.path.join(ROOT, 'src', 'infer.py'), sampled + ['--infer_top_p', '0'])
