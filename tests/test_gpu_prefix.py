"""Forced-prefix decoding on the device: the mask kernel (csrc/beam_prefix.hip) bit for bit against the numpy rule, and the
one executor loop from a prefix under every selection policy -- identities against the unforced decode, the float64
reference loop of tests/beam_prefix_ref.py, Decoder.score, batch independence, capture and replay, and infer.py."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import comic_amd._lib as L
from comic_amd import decoder as cdec
from comic_amd.decoder import BeamConstraints, BeamGroups, BeamPrefix, BeamRequired, BeamSampling, BeamTruncation
from tests import beam_prefix_ref as pref
from tests import beam_truncate_ref as tref
from tests.beam_constraints_ref import pack_bits
from tests.gpu_util import DEV, F32_RTOL, assert_close, dev, stream, sync
from tests.test_gpu_constraints import tiny_run  # noqa: F401  (the fixture: a one-epoch run on the tiny dataset)
from tests.test_gpu_ensemble import _features, _rand_params, _run, _spec_and_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_STEPS = 14
P_OP = 3


# ------------------------------------------------------------------ 1. the mask kernel ------------------------------------
def _op_case(B, W, V, t, seed):
    """A table of width 3 whose rows cycle through the lengths 3, 0, 1, 2 (B = 1: a full row), an entry outside [0, V) in
    the last image of a batch of three (never an index: that row is not forced at step 0), and every third row finished."""
    rng = np.random.default_rng(seed)
    pfx = np.full((B, P_OP), -1, np.int32)
    for b in range(B):
        n = (P_OP, 0, 1, 2)[b % 4]
        pfx[b, :n] = rng.integers(0, V, n)
    pfx[0, P_OP - 1] = V - 1                                       # the last bit below V, in a partly used last word
    if B == 3:
        pfx[2, 0] = V + 5
    finished = np.zeros(B * W, np.int32)
    finished[2::3] = 1
    if B * W == 1 and seed % 2:
        finished[:] = 1
    return pfx, finished


def _run_op(pfx, finished, incoming, t, B, W, V, has_bans):
    lib = L.load()
    d_bits = dev(incoming.view(np.int32))
    d_pfx, d_fin = dev(pfx), dev(finished)
    L.check(lib.comic_beam_prefix_mask(d_pfx.data_ptr(), d_fin.data_ptr(), d_bits.data_ptr(), t, B, W, V, pfx.shape[1],
                                       has_bans, stream()), 'beam_prefix_mask')
    sync()
    return d_bits.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('t', [0, P_OP - 1, P_OP])
@pytest.mark.parametrize('shape', [(1, 1, 33), (3, 3, 258), (2, 5, 9001), (1, 64, 65536), (3, 2, 100), (2, 3, 25599)])
def test_kernel_matches_the_rule_bit_for_bit(shape, t):
    """V = 33 and 258: a partly used last word, rows of 2 and 9 words (the 4-byte stores); 9001: 282 words, more than one
    word per lane; 65 536: 2048 words, the 16-byte stores, two per lane, a full last word; 100 and 25 599 (the word
    vocabulary): 4 and 800 words, the 16-byte stores with a partly used last word (4 and 31 bits)."""
    B, W, V = shape
    R, words = B * W, (V + 31) // 32
    rng = np.random.default_rng(7 * V + t)
    for seed in (0, 1):
        pfx, finished = _op_case(B, W, V, t, seed)
        # has_bans == 0: every word of every row is written, whatever the block held
        poison = np.full((R, words), 0xdeadbeef, np.uint32)
        want = pack_bits(pref.forced_mask(np.zeros((R, V), bool), pfx, finished, t, W))
        got = _run_op(pfx, finished, poison, t, B, W, V, 0)
        np.testing.assert_array_equal(got, want, err_msg='has_bans 0, seed %d' % seed)
        # has_bans == 1: the constraints' mask stands where a row is not forced (finished rows hold zeros, as
        # comic_beam_bans leaves them), and is replaced where it is
        cons = rng.random((R, V)) < 0.3
        cons[finished != 0] = False
        want = pack_bits(pref.forced_mask(cons, pfx, finished, t, W))
        got = _run_op(pfx, finished, pack_bits(cons), t, B, W, V, 1)
        np.testing.assert_array_equal(got, want, err_msg='has_bans 1, seed %d' % seed)
        forced, tok = pref.forced_rows(pfx, finished, t, W, V)
        assert forced.any() == (t < P_OP and (finished == 0).any())
        for r in np.nonzero(forced)[0]:
            assert not (got[r, tok[r] >> 5] >> (tok[r] & 31)) & 1 and int(np.unpackbits(got[r].view(np.uint8)).sum()) == V - 1
        assert not got[finished != 0].any(), 'a finished row bans nothing'


def test_kernel_refuses_bad_arguments():
    lib = L.load()
    buf = torch.zeros(4096, dtype=torch.int32, device=DEV)
    p = buf.data_ptr()
    for args, what in (((None, p, p, 0, 1, 1, 33, 2, 0), 'null pointer'), ((p, p, None, 0, 1, 1, 33, 2, 0), 'null pointer'),
                       ((p, p, p, 0, 1, 65, 33, 2, 0), 'bad shape'), ((p, p, p, 0, 1, 1, 65537, 2, 0), 'mask words'),
                       ((p, p, p, 0, 1, 1, 33, 0, 0), 'table width 0'), ((p, p, p, -1, 1, 1, 33, 2, 0), 'negative'),
                       ((p, p, p + 4, 0, 1, 1, 33, 2, 0), '16-byte aligned')):
        assert lib.comic_beam_prefix_mask(*args, stream()) != 0
        assert what in lib.comic_last_error().decode(), (what, lib.comic_last_error())
    sync()
    assert not bool(buf.any())


# ------------------------------------------------------------------ the whole decoder ------------------------------------
def _table(rows, P=None):
    P = P or max(1, max(len(r) for r in rows))
    ids = np.full((len(rows), P), -1, np.int32)
    for b, r in enumerate(rows):
        ids[b, :len(r)] = r
    return ids


def _starts_with(res, b, slot, row):
    n = int((np.asarray(row) >= 0).sum())
    return res['predicted_ids'][:n, b, slot].tolist() == [int(x) for x in row[:n]]


@functools.lru_cache(maxsize=None)
def _decoder(seed=61, **geo):
    spec, cfg = _spec_and_cfg(**geo)
    p = _rand_params(cfg, seed, 3.0)
    return spec, cfg, p, cdec.Decoder(spec, p, DEV)


# ------------------------------------------------------------------ 2. greedy identity ------------------------------------
def test_forcing_the_greedy_caption_changes_nothing():
    """W = 1: forcing the first k tokens of the caption the decode emits anyway (k ragged over the batch, 0 included) gives
    the unforced decode of the same executor to the bit -- the forced steps rank the one candidate by the same total."""
    fm, im = _features()
    spec, cfg, p, dec = _decoder()
    ens = cdec.EnsembleDecoder([dec])
    base = ens.beam_search(dev(fm), dev(im), 1, MAX_STEPS, use_graph=False)
    ks = np.minimum([3, 0, 2], base['lengths'][:, 0] - 1)             # (never the <EOS> itself)
    assert ks.tolist() == [3, 0, 1], base['lengths']                  # (checked on the CPU: the captions hold 14, 1, 2 tokens)
    rows = [base['step_ids'][:k, b, 0].tolist() for b, k in enumerate(ks)]
    res = ens.beam_search(dev(fm), dev(im), 1, MAX_STEPS, use_graph=False, prefix=BeamPrefix(_table(rows)))
    for k in ('step_ids', 'parent_ids', 'predicted_ids', 'lengths', 'scores'):
        np.testing.assert_array_equal(res[k], base[k], err_msg=k)
    np.testing.assert_array_equal(res['log_probs'], base['scores'][-1])
    for b, k in enumerate(ks):
        assert res['prefix_log_prob'][b, 0] == (base['scores'][k - 1, b, 0] if k else 0.0)


# ------------------------------------------------------------------ 3. sampled identity -----------------------------------
N_DEC, TEMP, NSEED = 4, 0.8, 2
# the first 3, 0 and 1 tokens of the slot-0 samples of the unforced decode: untruncated, and under top-5 / top-p 0.9
SAMPLED_TABLES = {False: [[72, 179, 36], [-1, -1, -1], [234, -1, -1]], True: [[221, 92, 199], [-1, -1, -1], [33, -1, -1]]}


@pytest.mark.parametrize('trc', [None, BeamTruncation(5, 0.9)], ids=['untruncated', 'top5-p0.9'])
def test_forcing_a_sample_reproduces_its_chain(trc):
    """n = 4 chains at temperature 0.8, noise seed 2: forcing the first k tokens of each image's slot-0 sample makes slot 0
    reproduce its ids and log-probabilities to the bit (the noise is keyed by seed, image, slot, step and token, and the
    forced token keeps the model's own log-probability), and every slot of every image starts with the prefix.  Under
    top-5 / top-p 0.9 the same.  Then every slot -- ids, parents, lengths exactly, scores and log_probs at the fp32 bar --
    against the float64 reference loop run from the same table.  Checked on the CPU: the tables are SAMPLED_TABLES, both
    references run 14 steps, rank-gap margins 243.09 and 219.61; under the truncation no step has a token in the band
    between must_keep and must_drop, so the device mask is determined."""
    fm, im = _features()
    spec, cfg, p, dec = _decoder()
    kw = dict(want_attention=False, use_graph=False, sampling=BeamSampling(TEMP, NSEED), truncation=trc)
    base = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, **kw)
    ks = np.minimum([3, 0, 2], base['lengths'][:, 0] - 1)
    assert ks.tolist() == [3, 0, 1], base['lengths']
    table = _table([base['step_ids'][:k, b, 0].tolist() for b, k in enumerate(ks)])
    res = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, prefix=BeamPrefix(table), **kw)
    assert (res['parent_ids'] == np.arange(N_DEC)).all()
    T = min(res['step_ids'].shape[0], base['step_ids'].shape[0])
    assert T >= int(base['lengths'][:, 0].max())                      # slot 0's whole chain lies inside both results
    np.testing.assert_array_equal(res['step_ids'][:T, :, 0], base['step_ids'][:T, :, 0])
    np.testing.assert_array_equal(res['scores'][:T, :, 0], base['scores'][:T, :, 0])
    np.testing.assert_array_equal(res['lengths'][:, 0], base['lengths'][:, 0])
    np.testing.assert_array_equal(res['log_probs'][:, 0], base['log_probs'][:, 0])
    for b in range(fm.shape[0]):
        for w in range(N_DEC):
            assert _starts_with(res, b, w, table[b]), (b, w)
            assert res['lengths'][b, w] > ks[b]
    assert not np.array_equal(res['step_ids'][:, :, 1:], base['step_ids'][:res['step_ids'].shape[0], :, 1:])    # the others moved
    np.testing.assert_array_equal(res['prefix_log_prob'][1], 0.0)
    for b in np.nonzero(ks)[0]:                                       # a chain's prefix total: its score after step k - 1
        np.testing.assert_array_equal(res['prefix_log_prob'][b], res['scores'][ks[b] - 1, b])
    # every slot against the float64 reference loop of the same table: the sampled selection under the forced mask and,
    # with a truncation, under the top-k / top-p sandwich of tests/beam_truncate_ref.py on top of it
    assert table.tolist() == SAMPLED_TABLES[trc is not None]
    tkw = dict() if trc is None else dict(top_k=trc.top_k, top_p=trc.top_p)
    ref = pref.prefixed_reference([(p, cfg)], np.ones(1, np.float32), fm, im, N_DEC, MAX_STEPS, table, policy='samples',
                                  seed=NSEED, temperature=TEMP, **tkw)
    print('reference rank-gap margin over %d steps: %.2f (must exceed 1); largest band %d, both ends of the sandwich agree: %s'
          % (ref['step_ids'].shape[0], ref['margin'], ref['band'], ref['sandwich_agrees']))
    assert ref['margin'] > 1.0 and ref['sandwich_agrees'] and ref['band'] <= tref.BAND_CAP
    assert res['step_ids'].shape[0] == ref['step_ids'].shape[0]                # steps_executed
    for k in ('step_ids', 'parent_ids', 'lengths'):
        np.testing.assert_array_equal(res[k], ref[k], err_msg=k)
    assert_close(res['scores'], ref['scores'], F32_RTOL, 'scores')
    assert_close(res['log_probs'], ref['log_probs'], F32_RTOL, 'final log_probs')
    for b in range(fm.shape[0]):
        for w in range(N_DEC):
            assert pref.captions(res, b, w) == pref.trace(ref, b, w)


# ------------------------------------------------------------------ 4. against the float64 reference loops ----------------
PFX = [[17, 40, 5], [200], []]                    # ragged, 0 included; image 0's holds its required word 40
PFX_BIG = [[17, 4000, 8999], [200], []]
# name -> (geometry, prefix rows, beam, reference keywords, decoder keywords).  Checked on the CPU with parameter seed 61:
# the rank-gap margins of the float64 reference over the steps behind the prefixes are
#   beam-258 8.71 (14 steps), groups-258 5.18 (14), banks-258 26.50 (14), beam-9001 10.59 (5 steps: every beam ends),
#   groups-9001 11.95 (5), banks-9001 16.06 (5), constraints 2.56 (14), ensemble (seeds 38, 39) 34.53 (14).
CASES = {
    'beam-258': (dict(), PFX, 3, dict(policy='beam'), dict()),
    'groups-258': (dict(), PFX, 4, dict(policy='groups', G=2, lam=0.5), dict(groups=BeamGroups(2, 0.5))),
    'banks-258': (dict(), PFX, 4, dict(policy='banks', req=[[[40]], [[9]], [[-1]]], S=1),
                  dict(required=BeamRequired([[[40]], [[9]], [[-1]]]))),
    'beam-9001': (dict(V=9001), PFX_BIG, 3, dict(policy='beam'), dict()),
    'groups-9001': (dict(V=9001), PFX_BIG, 4, dict(policy='groups', G=2, lam=0.5), dict(groups=BeamGroups(2, 0.5))),
    'banks-9001': (dict(V=9001), PFX_BIG, 4, dict(policy='banks', req=[[[4000]], [[9]], [[-1]]], S=1),
                   dict(required=BeamRequired([[[4000]], [[9]], [[-1]]]))),
}


def _check_decode(res, ref, table):
    """Every slot with a finite score: ids, parents and lengths exact, scores and final log-probabilities at the fp32 bar;
    the slots the rule leaves at -inf are -inf; every caption of a finite slot starts with its image's prefix."""
    assert res['step_ids'].shape[0] == ref['step_ids'].shape[0]                # steps_executed
    fin = np.isfinite(ref['scores'])
    assert fin.any(axis=2).all() and not fin[0].all(), 'the case has no -inf slot at its first step'
    np.testing.assert_array_equal(res['step_ids'][fin], ref['step_ids'][fin])
    np.testing.assert_array_equal(res['parent_ids'][fin], ref['parent_ids'][fin])
    np.testing.assert_array_equal(res['lengths'][fin[-1]], ref['lengths'][fin[-1]])
    assert np.isneginf(res['scores'][~fin]).all() and np.isneginf(ref['scores'][~fin]).all()
    assert_close(np.where(fin, res['scores'], 0), np.where(fin, ref['scores'], 0), F32_RTOL, 'scores')
    assert_close(np.where(fin[-1], res['log_probs'], 0), np.where(fin[-1], ref['log_probs'], 0), F32_RTOL, 'log_probs')
    assert np.isneginf(res['log_probs'][~fin[-1]]).all()
    B, W = fin.shape[1:]
    for b in range(B):
        for w in np.nonzero(fin[-1, b])[0]:
            assert _starts_with(res, b, w, table[b]), (b, w, res['predicted_ids'][:, b, w])
            assert pref.captions(res, b, w) == pref.trace(ref, b, w)
    # no -inf slot is an ancestor of a slot with a finite final score
    alive = fin[-1].copy()
    for t in range(fin.shape[0] - 1, -1, -1):
        assert fin[t][alive].all()
        nxt = np.zeros_like(alive)
        for b in range(B):
            nxt[b, res['parent_ids'][t, b][alive[b]]] = True
        alive = nxt


@pytest.mark.parametrize('name', list(CASES))
def test_decode_matches_the_float64_reference(name):
    """V = 258 ranks in the one-workgroup step, V = 9001 in the split step (8 chunks).  Plain beam and groups: the first
    slot (of each group) carries the prefix, the others hold -inf until the first free step; banks: image 0's prefix holds
    its required word, which counts as produced."""
    geo, rows, W, rkw, dkw = CASES[name]
    fm, im = _features()
    spec, cfg, p, dec = _decoder(**geo)
    table = _table(rows)
    ref = pref.prefixed_reference([(p, cfg)], np.ones(1, np.float32), fm, im, W, MAX_STEPS, table, **rkw)
    print('%s: reference rank-gap margin over %d steps: %.2f (must exceed 1)' % (name, ref['step_ids'].shape[0], ref['margin']))
    assert ref['margin'] > 1.0
    res = dec.beam_search(dev(fm), dev(im), W, MAX_STEPS, want_attention=False, use_graph=False, prefix=BeamPrefix(table), **dkw)
    _check_decode(res, ref, table)
    if 'required' in dkw:
        from tests.beam_required_ref import result_rule
        best, met = result_rule(ref['scores'][-1], 2, 1)
        np.testing.assert_array_equal(res['best_slot'], best)
        np.testing.assert_array_equal(res['met'], met)
        assert res['met'][0] == 1                                     # image 0's word: produced by the prefix itself
        assert np.isneginf(res['scores'][-1][0, 0]), 'image 0 can no longer be in the bank of nothing produced'


def test_the_prefix_wins_over_the_constraints_inside_it():
    """min_length 6, no repeated bigram, 7 and 155 suppressed.  Image 0's prefix 5 6 5 6 repeats a bigram, image 1's starts
    with the suppressed 7: both are emitted, and from step len on the constraints hold -- no 7 or 155, no <EOS> before
    step 6, and no bigram that the caption (prefix included: the histories count it) already holds.  Checked on the CPU:
    14 steps, margin 2.56."""
    kw = dict(no_repeat_ngram=2, min_length=6, suppress=(7, 155))
    rows = [[5, 6, 5, 6], [7, 30], []]
    fm, im = _features()
    spec, cfg, p, dec = _decoder()
    table = _table(rows)
    ref = pref.prefixed_reference([(p, cfg)], np.ones(1, np.float32), fm, im, 3, MAX_STEPS, table, policy='beam', **kw)
    print('reference rank-gap margin %.2f' % ref['margin'])
    assert ref['margin'] > 1.0 and ref['step_ids'].shape[0] == MAX_STEPS
    res = dec.beam_search(dev(fm), dev(im), 3, MAX_STEPS, want_attention=False, constraints=BeamConstraints(**kw),
                          prefix=BeamPrefix(table))
    _check_decode(res, ref, table)
    for b in range(3):
        for w in range(3):
            cap, n = pref.captions(res, b, w), len(rows[b])
            assert cap[:n] == rows[b] and len(cap) > 6 and spec.end_id not in cap[:6]
            assert 7 not in cap[n:] and 155 not in cap[n:]
            for i in range(max(n, 1), len(cap)):
                assert (cap[i - 1], cap[i]) not in set(zip(cap[:i - 1], cap[1:i])), 'a bigram repeats behind the prefix: %r' % (cap,)


def test_ensemble_of_two_members():
    """Two members with different head counts, weights [0.6, 0.4].  Checked on the CPU: 14 steps, margin 34.53."""
    fm, im = _features()
    members = []
    for seed, geo in ((38, dict()), (39, dict(H=4))):
        spec, cfg = _spec_and_cfg(**geo)
        members.append((spec, cfg, _rand_params(cfg, seed, 3.0)))
    wts = [0.6, 0.4]
    table = _table(PFX)
    ref = pref.prefixed_reference([(p, cfg) for _, cfg, p in members], np.asarray(wts, np.float32), fm, im, 3, MAX_STEPS, table)
    print('reference rank-gap margin %.2f' % ref['margin'])
    assert ref['margin'] > 1.0
    ens = cdec.EnsembleDecoder([cdec.Decoder(spec, p, DEV) for spec, _, p in members], wts)
    _check_decode(ens.beam_search(dev(fm), dev(im), 3, MAX_STEPS, prefix=BeamPrefix(table)), ref, table)


# ------------------------------------------------------------------ 5. Decoder.score ---------------------------------------
@pytest.mark.parametrize('grp', [None, BeamGroups(2, 0.5)], ids=['beam', 'groups'])
@pytest.mark.parametrize('lpw', [0.0, 0.7])
def test_decoder_score_reproduces_both_log_probabilities(lpw, grp):
    """log_probs is the model's log p(prefix + continuation | image) and prefix_log_prob its share of the forced steps:
    Decoder.score of the whole captions gives the first as log_prob and the second as the sum of the first len token
    log-probabilities.  With a length penalty the result's scores are penalised and both come out unpenalised; with two
    groups at diversity 0.5 the second group's carrier emits the forced token behind the first's, so its scores carry the
    diversity penalty, which prefix_log_prob takes out again."""
    fm, im = _features()
    spec, cfg, p, dec = _decoder()
    table = _table(PFX)
    W = 3 if grp is None else 4
    res = dec.beam_search(dev(fm), dev(im), W, MAX_STEPS, want_attention=False, length_penalty_weight=lpw, groups=grp,
                          prefix=BeamPrefix(table))
    T, B = res['predicted_ids'].shape[:2]
    ok = np.isfinite(res['scores'][-1])
    assert ok[:, 0].all()
    if grp is not None:                                               # the penalty is there to be taken out
        n0 = len(PFX[0])
        assert ok[:, 2].all() and (res['step_ids'][n0 - 1, 0, 2] == res['step_ids'][n0 - 1, 0, 0] == PFX[0][-1])
    caps = np.full((B * W, T + 1), -1, np.int64)
    caps[:, 0] = spec.start_id
    for b in range(B):
        for w in range(W):
            cap = pref.captions(res, b, w if ok[b, w] else 0)         # (a dead slot: scored as slot 0, not compared)
            caps[b * W + w, 1:1 + len(cap)] = cap
    rep = lambda a: dev(np.repeat(a, W, axis=0))                      # noqa: E731
    sc = dec.score(rep(fm), rep(im), caps, use_graph=False)
    total = sc['log_prob'].cpu().numpy().reshape(B, W)
    tok = sc['token_log_probs'].cpu().numpy().reshape(B, W, -1)
    n = pref.prefix_lengths(table)
    forced = np.stack([tok[b, :, :n[b]].sum(axis=1) for b in range(B)])
    assert_close(np.where(ok, res['log_probs'], 0), np.where(ok, total, 0), F32_RTOL, 'log_probs against Decoder.score')
    assert_close(np.where(ok, res['prefix_log_prob'], 0), np.where(ok, forced, 0), F32_RTOL, 'prefix_log_prob')
    assert (res['prefix_log_prob'][2] == 0).all() and (res['prefix_log_prob'][:2, 0] < 0).all()


# ------------------------------------------------------------------ 6. batch independence ---------------------------------
def test_an_image_does_not_see_its_neighbours_prefixes():
    """The image with the empty row of a mixed batch decodes to the bits of its unprefixed decode on the same executor, and
    an image decodes to the same bits alone and in the batch of 3."""
    fm, im = _features()
    spec, cfg, p, dec = _decoder()
    ens = cdec.EnsembleDecoder([dec])
    table = _table(PFX)
    W = 3
    mixed = ens.beam_search(dev(fm), dev(im), W, MAX_STEPS, use_graph=False, prefix=BeamPrefix(table))
    plain = ens.beam_search(dev(fm), dev(im), W, MAX_STEPS, use_graph=False)
    T = min(mixed['step_ids'].shape[0], plain['step_ids'].shape[0])
    for k in ('step_ids', 'parent_ids', 'scores'):
        np.testing.assert_array_equal(mixed[k][:T, 2], plain[k][:T, 2], err_msg='the image without a prefix: ' + k)
    np.testing.assert_array_equal(mixed['lengths'][2], plain['lengths'][2])
    assert not np.array_equal(mixed['step_ids'][:T, 0], plain['step_ids'][:T, 0])
    for b in range(3):
        alone = ens.beam_search(dev(fm[b:b + 1]), dev(im[b:b + 1]), W, MAX_STEPS, use_graph=False,
                                prefix=BeamPrefix(table[b:b + 1]))
        Ta = alone['step_ids'].shape[0]
        assert Ta <= mixed['step_ids'].shape[0]
        fin = np.isfinite(alone['scores'][:, 0])
        for k in ('step_ids', 'parent_ids', 'scores'):
            np.testing.assert_array_equal(alone[k][:, 0][fin], mixed[k][:Ta, b][fin], err_msg='image %d alone: %s' % (b, k))
        np.testing.assert_array_equal(alone['lengths'][0][fin[-1]], mixed['lengths'][b][fin[-1]])


# ------------------------------------------------------------------ 7. capture and replay ---------------------------------
def test_one_context_and_one_graph_serve_every_table_of_a_width():
    fm, im = _features()
    spec, cfg, p = _decoder()[:3]
    dec = cdec.Decoder(spec, p, DEV)                                  # (its own contexts: this test counts them)
    W = 3
    a, b = BeamPrefix(_table(PFX)), BeamPrefix(_table([[9], [33, 12, 101], [64, 2]]))
    run = lambda pfx, **kw: dec.beam_search(dev(fm), dev(im), W, MAX_STEPS, want_attention=True, prefix=pfx, **kw)    # noqa: E731
    before = dec.beam_search(dev(fm), dev(im), W, MAX_STEPS, want_attention=False)
    assert '_self_ensemble' not in dec.__dict__                       # prefix=None: the plain decode's own executor
    eager_a, eager_b = run(a, use_graph=False), run(b, use_graph=False)
    ctxs = dec._self_ensemble._ctxs
    assert len(ctxs) == 1 and next(iter(ctxs.values())).graph is None
    captured = run(a)
    graph = next(iter(ctxs.values())).graph
    assert graph is not None
    replay_a, replay_b = run(a), run(b)
    assert len(ctxs) == 1 and next(iter(ctxs.values())).graph is graph, 'a new table must not build or capture anything'
    for k in ('step_ids', 'parent_ids', 'predicted_ids', 'lengths', 'scores', 'log_probs', 'prefix_log_prob', 'attn_hist'):
        np.testing.assert_array_equal(captured[k], eager_a[k], err_msg='capture: ' + k)
        np.testing.assert_array_equal(replay_a[k], eager_a[k], err_msg='replay: ' + k)
        np.testing.assert_array_equal(replay_b[k], eager_b[k], err_msg='replay of the other table: ' + k)
    for w in (0,):
        assert all(_starts_with(replay_b, i, w, b.ids[i]) for i in range(3))
    assert not np.array_equal(eager_a['predicted_ids'][:3], eager_b['predicted_ids'][:3])
    fetch = dec.beam_search_ids(dev(fm), dev(im), W, MAX_STEPS, prefix=b)     # the ids alone: the same context and graph
    np.testing.assert_array_equal(fetch(), eager_b['predicted_ids'])
    assert len(ctxs) == 1 and next(iter(ctxs.values())).graph is graph
    wider = run(BeamPrefix(_table(PFX, P=4)))                         # another width is another context
    assert len(ctxs) == 2
    np.testing.assert_array_equal(wider['predicted_ids'], eager_a['predicted_ids'])
    after = dec.beam_search(dev(fm), dev(im), W, MAX_STEPS, want_attention=False, prefix=None)
    assert len(ctxs) == 2 and sorted(after) == sorted(before)
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg='prefix=None: ' + k)


def test_refused_on_the_host_before_anything_is_built():
    fm, im = _features()
    spec, cfg, p = _decoder()[:3]
    dec = cdec.Decoder(spec, p, DEV)
    for rows, what in (([[1], [2]], 'the table holds 2 images, the batch 3'), ([[257], [], []], 'end_id'),
                       ([[1] * MAX_STEPS, [], []], 'max_tokens 14')):
        with pytest.raises(ValueError, match=what):
            dec.beam_search(dev(fm), dev(im), 3, MAX_STEPS, prefix=BeamPrefix(_table(rows)))
    assert '_self_ensemble' not in dec.__dict__


# ------------------------------------------------------------------ 8. infer.py --------------------------------------------
def test_infer_cli_prefix_and_prefix_file(tiny_run, tmp_path):  # noqa: F811
    """--infer_prefix and --infer_prefix_file on the tiny dataset (radix tokens, one token per word): each writes a directory
    of its own with both files, and every caption starts with its prefix; a word outside the vocabulary is an error for the
    one flag and cuts the prefix for the file."""
    ds, run_dir, ckpt = tiny_run
    num = os.path.basename(ckpt)[len('model_compact-'):-len('.npz')]
    common = ['--infer_checkpoints_dir', run_dir, '--dataset_dir', ds, '--infer_set', 'test', '--batch_size_infer', '2',
              '--get_metric_score', '', '--infer_checkpoints', num]
    infer = os.path.join(ROOT, 'src', 'infer.py')
    plain_dir = os.path.join(run_dir, 'infer_test_beam_3_lpen_0.0')
    with pytest.raises(ValueError, match="'zebra' is outside the vocabulary"):
        _run(infer, common + ['--infer_prefix', 'a zebra'])
    with pytest.raises(ValueError, match='not both'):
        _run(infer, common + ['--infer_prefix', 'a dog', '--infer_prefix_file', 'x.json'])
    assert not [d for d in os.listdir(run_dir) if '_pfx' in d]                   # refused before anything was written
    _run(infer, common + ['--infer_prefix', 'a dog on'])
    out = plain_dir + '_pfx_a-dog-on'
    assert not os.path.exists(plain_dir)
    caps = json.load(open(os.path.join(out, 'captions___%s.json' % num)))
    rows = json.load(open(os.path.join(out, 'caption_prefix___%s.json' % num)))
    assert [r['image_id'] for r in rows] == [c['image_id'] for c in caps] == [1, 2, 3, 4]
    for cap, r in zip(caps, rows):
        assert r['prefix'] == ['a', 'dog', 'on'] and r['cut'] == []
        assert cap['caption'].split()[:3] == ['a', 'dog', 'on'], cap
        assert np.isfinite(r['log_prob']) and r['log_prob'] <= r['prefix_log_prob'] < 0
    starts = tmp_path / 'starts.json'
    starts.write_text(json.dumps({'1': 'the cat zebra on', 'COCO_test2014_000000000002.jpg': ['red', 'bench']}))
    _run(infer, common + ['--infer_prefix_file', str(starts)])
    out = plain_dir + '_pfx_starts'
    caps = json.load(open(os.path.join(out, 'captions___%s.json' % num)))
    rows = json.load(open(os.path.join(out, 'caption_prefix___%s.json' % num)))
    assert [r['prefix'] for r in rows] == [['the', 'cat'], ['red', 'bench'], [], []]
    assert [r['cut'] for r in rows] == [['zebra', 'on'], [], [], []]
    for cap, r in zip(caps, rows):
        assert cap['caption'].split()[:len(r['prefix'])] == r['prefix'], cap
        assert (r['prefix_log_prob'] == 0) == (not r['prefix'])
