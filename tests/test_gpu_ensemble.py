"""Ensemble beam search on the GPU: the step operator (comic_beam_step_ensemble) against a float64 restatement of its
formula, the whole decoder (decoder.EnsembleDecoder -> comic_decoder_beam_ensemble) against Decoder.beam_search and against
a reference loop built from the oracle's decoder pieces, and `infer.py --infer_ensemble` on the tiny dataset.

Ids are compared exactly, and only claimed where the float64 reference separates consecutive ranks 1 ... W + 1 by more than
GAP * max(1, |score|) -- an order above the fp32 log-sum-exp error at these vocabulary sizes.  The seeds below were chosen on
the CPU so that the reference meets that gap in EVERY entry of every case; each test asserts it (no entry is excused)."""
import ctypes as C
import functools
import glob
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import comic_amd._lib as L
from comic_amd import decoder as cdec
from oracle import beam_ref, decoder_ref as dr
from tests.gpu_util import DEV, F32_RTOL, assert_close, dev, stream, sync

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 1e-4
F32_MIN = float(np.finfo(np.float32).min)
POISON = 0x7f7f7f7f


# ------------------------------------------------------------------ float64 reference of one step ------------------
def ref_step_lp(logits, wts):
    """lp [B,W,V] = log sum_m wt_m softmax(logits_m) in float64: a_m log-softmax, A = max over the members that count,
    lp = A + log sum_m wt_m exp(a_m - A), members in order."""
    x = np.asarray(logits, np.float64)
    a = x - x.max(axis=-1, keepdims=True)
    a = a - np.log(np.exp(a).sum(axis=-1, keepdims=True))
    live = [m for m in range(len(wts)) if wts[m] > 0]
    A = a[live].max(axis=0)
    s = np.zeros_like(A)
    for m in live:
        s += np.float64(wts[m]) * np.exp(a[m] - A)
    return A + np.log(s)


def ref_select(lp, log_probs, finished, lengths, end_id, lpw):
    """The bookkeeping of oracle/beam_ref.beam_search_decode on a given step distribution, in float64.
    -> dict(word, parent, scores, log_probs, finished, lengths, margin); margin = min over entries and ranks 1..W of
    (gap to the next rank) / (GAP * max(1, |score|)): > 1 means every id is claimed."""
    B, W, V = lp.shape
    fin = np.asarray(finished, bool)
    fin_row = np.full(V, F32_MIN, np.float64)
    fin_row[end_id] = 0
    step = np.where(fin[:, :, None], fin_row[None, None, :], lp)
    total = np.asarray(log_probs, np.float64)[:, :, None] + step
    flat_total = total.reshape(B, W * V)
    if lpw != 0:
        add = np.ones(V, np.int64)
        add[end_id] = 0
        new_len = lengths[:, :, None] + add[None, None, :] * (~fin)[:, :, None]
        flat = (total / ((5.0 + new_len) / 6.0) ** np.float64(np.float32(lpw))).reshape(B, W * V)
    else:
        flat = flat_total
    order = np.argsort(-flat, axis=1, kind='stable')[:, :W + 1]
    top = np.take_along_axis(flat, order, axis=1)
    gaps = top[:, :-1] - top[:, 1:]
    margin = float((gaps / (GAP * np.maximum(1.0, np.abs(top[:, :-1])))).min())
    order = order[:, :W]
    bidx = np.arange(B)[:, None]
    word, parent = (order % V).astype(np.int32), (order // V).astype(np.int32)
    prev_fin = fin[bidx, parent]
    return dict(word=word, parent=parent, scores=top[:, :W], log_probs=np.take_along_axis(flat_total, order, axis=1),
                finished=(prev_fin | (word == end_id)).astype(np.int32),
                lengths=lengths[bidx, parent] + (~prev_fin).astype(np.int64), margin=margin)


# ------------------------------------------------------------------ operator level -----------------------------------
# (n, B, W, V): smallest case; radix vocabulary; split form with V not divisible by its 8 chunks; maximum member count
SHAPES = [(1, 2, 3, 17), (3, 3, 3, 258), (2, 2, 5, 9001), (8, 1, 2, 300)]
STEP_CASES = [(s, state, lpw) for s in SHAPES for state in ('init', 'mid') for lpw in (0.0, 0.7)]
# the rescanning form of the split step: 8 chunks of 1126 columns, 5 per thread x 9 beams = 45 > 40 register slots
STEP_CASES.append(((2, 2, 9, 9001), 'mid', 0.0))
STEP_SEED = 0             # checked on the CPU: the float64 reference of every case meets the rank gap at twice the bar


@functools.lru_cache(maxsize=None)
def step_case(shape, state, lpw, seed=None):
    n, B, W, V = shape
    rng = np.random.default_rng(STEP_SEED if seed is None else seed)
    logits = (2.0 * rng.standard_normal((n, B, W, V))).astype(np.float32)
    wts = np.ones(1, np.float32) if n == 1 else rng.dirichlet(np.ones(n)).astype(np.float32)
    end_id = V - 1
    if state == 'init':
        log_probs = np.full((B, W), -np.inf, np.float32)
        log_probs[:, 0] = 0
        finished = np.ones((B, W), np.int32)
        finished[:, 0] = 0
        lengths = np.zeros((B, W), np.int64)
    else:                                   # mid-decode: one finished beam per entry
        log_probs = -rng.uniform(1.0, 6.0, (B, W)).astype(np.float32)
        finished = np.zeros((B, W), np.int32)
        finished[np.arange(B), rng.integers(0, W, B)] = 1
        lengths = rng.integers(1, 7, (B, W)).astype(np.int64)
    ref = ref_select(ref_step_lp(logits, wts), log_probs, finished, lengths, end_id, lpw)
    return dict(logits=logits, wts=wts, end_id=end_id, log_probs=log_probs, finished=finished, lengths=lengths, ref=ref)


def run_step(logits, wts, log_probs, finished, lengths, end_id, lpw, workspace=True):
    lib = L.load()
    n, B, W, V = logits.shape
    d_lg, d_lp, d_fin, d_len = dev(logits), dev(log_probs), dev(finished), dev(lengths)
    word = torch.full((B, W), -1, dtype=torch.int32, device=DEV)
    parent = torch.full((B, W), -1, dtype=torch.int32, device=DEV)
    scores = torch.zeros((B, W), dtype=torch.float32, device=DEV)
    nbytes = int(lib.comic_beam_step_ensemble_workspace(n, B, W, V))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ws_ptr, ws_bytes = (ws.data_ptr(), nbytes) if workspace else (None, 0)
    wt = (C.c_float * n)(*[float(w) for w in wts])
    L.check(lib.comic_beam_step_ensemble(d_lg.data_ptr(), wt, n, d_lp.data_ptr(), d_fin.data_ptr(), d_len.data_ptr(),
                                         word.data_ptr(), parent.data_ptr(), scores.data_ptr(), B, W, V, end_id, float(lpw),
                                         ws_ptr, ws_bytes, stream()), 'beam_step_ensemble')
    sync()
    return dict(word=word.cpu().numpy(), parent=parent.cpu().numpy(), scores=scores.cpu().numpy(),
                log_probs=d_lp.cpu().numpy(), finished=d_fin.cpu().numpy(), lengths=d_len.cpu().numpy(),
                split=int(lib.comic_beam_step_ensemble_path()))


@pytest.mark.parametrize('shape,state,lpw', STEP_CASES)
def test_ensemble_step_matches_float64(shape, state, lpw):
    c = step_case(shape, state, lpw)
    ref = c['ref']
    print('reference rank-gap margin %.2f (must exceed 1)' % ref['margin'])
    assert ref['margin'] > 1.0, 'the seed of this case does not separate the ranks of the float64 reference'
    got = run_step(c['logits'], c['wts'], c['log_probs'], c['finished'], c['lengths'], c['end_id'], lpw)
    # the split form runs exactly where the rule says: no penalty, W*V >= 8192, at least two chunks
    assert got['split'] == (1 if (shape[3] == 9001 and lpw == 0.0) else 0)
    for k in ('word', 'parent', 'finished', 'lengths'):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert_close(got['scores'], ref['scores'], F32_RTOL, 'scores')
    assert_close(got['log_probs'], ref['log_probs'], F32_RTOL, 'new log_probs')


@pytest.mark.parametrize('state', ['init', 'mid'])
def test_one_member_of_weight_1_is_comic_beam_step(state):
    """n = 1, weights [1.0], no workspace against comic_beam_step: the logits are finite, so the ensemble's
    a + logf(1 * expf(0)) is a exactly and the outputs and the new state are equal to the bit."""
    c = step_case((1, 3, 3, 258), state, 0.0)
    ens = run_step(c['logits'], [1.0], c['log_probs'], c['finished'], c['lengths'], c['end_id'], 0.0, workspace=False)
    B, W, V = c['logits'].shape[1:]
    d_lg, d_lp, d_fin, d_len = dev(c['logits'][0]), dev(c['log_probs']), dev(c['finished']), dev(c['lengths'])
    word = torch.full((B, W), -1, dtype=torch.int32, device=DEV)
    parent = torch.full((B, W), -1, dtype=torch.int32, device=DEV)
    scores = torch.zeros((B, W), dtype=torch.float32, device=DEV)
    L.check(L.load().comic_beam_step(d_lg.data_ptr(), d_lp.data_ptr(), d_fin.data_ptr(), d_len.data_ptr(), word.data_ptr(),
                                     parent.data_ptr(), scores.data_ptr(), B, W, V, c['end_id'], stream()), 'beam_step')
    sync()
    one = dict(word=word, parent=parent, scores=scores, log_probs=d_lp, finished=d_fin, lengths=d_len)
    for k, v in one.items():
        np.testing.assert_array_equal(ens[k], v.cpu().numpy(), err_msg=k)


@pytest.mark.parametrize('shape', [(2, 3, 3, 258), (2, 2, 5, 9001)])
def test_zero_weight_member_is_member_0_alone(shape):
    """Weights [1, 0]: the ids (and, the sum being exp(0) = 1, the scores to the bit) of member 0 on its own."""
    n, B, W, V = shape
    for state in ('init', 'mid'):
        c = step_case((n, B, W, V), state, 0.0, seed=7)
        both = run_step(c['logits'], [1.0, 0.0], c['log_probs'], c['finished'], c['lengths'], c['end_id'], 0.0)
        alone = run_step(c['logits'][:1], [1.0], c['log_probs'], c['finished'], c['lengths'], c['end_id'], 0.0)
        for k in ('word', 'parent', 'finished', 'lengths', 'scores', 'log_probs'):
            np.testing.assert_array_equal(both[k], alone[k], err_msg=k)


# ------------------------------------------------------------------ whole decoder --------------------------------------
def _spec_and_cfg(**kw):
    base = dict(D=128, E=64, V=258, C=192, Cg=192, H=8, M=25)      # the smallest geometry of tests/test_gpu_path.py
    base.update(kw)
    spec = cdec.DecoderSpec(**base)
    cfg = dr.DecoderConfig(rnn_size=spec.D, rnn_word_size=spec.E, attn_num_heads=spec.H,
                           cnn_fm_projection=spec.fm_projection, attn_alignment_method=spec.method,
                           attn_probability_fn=spec.prob, attn_context_layer=spec.context_layer,
                           rnn_init_method=spec.init_method, token_type=spec.token_type, softmax_size=spec.V,
                           fm_channels=spec.C, im_embed_size=spec.Cg, start_id=spec.start_id, end_id=spec.end_id,
                           rnn_name=spec.rnn_name)
    return spec, cfg


def _rand_params(cfg, seed, eos_bias):
    p = dr.init_params(cfg, seed)
    rng = np.random.default_rng(seed + 100)
    for k in p:
        if k in ('b', 'b_o', 'ln_b', 'b_c') or (k.startswith('cln_') and k.endswith('b')):
            p[k] = (0.1 * rng.standard_normal(p[k].shape)).astype(np.float32)
        if k == 'ln_g' or (k.startswith('cln_') and k.endswith('g')):
            p[k] = (1 + 0.1 * rng.standard_normal(p[k].shape)).astype(np.float32)
    # random projections give nearly flat word distributions, whose ranks no fp32 kernel could be held to: a wider output
    # projection makes them peaked, and the EOS bias then decides how long the beams live
    p['W_o'] = (p['W_o'] * np.float32(12.0)).astype(np.float32)
    p['b_o'][cfg.end_id] = eos_bias
    return p


B_DEC, W_DEC, MAX_STEPS = 3, 3, 14
MIXED_KW = (dict(), dict(H=4), dict(rnn_name='LN_LSTM'))
MIXED_SEED = 5            # members get MIXED_SEED, + 1, + 2.  Checked on the CPU: with EOS_BIAS the reference runs all 14
MIXED_WEIGHTS = [0.5, 0.3, 0.2]   # steps with finished and live beams side by side, rank-gap margin 7; with EOS_BIAS_EARLY
EOS_BIAS, EOS_BIAS_EARLY = 3.0, 5.0   # every beam ends after 2 steps


def _features(seed=21):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B_DEC, 25, 192)).astype(np.float32), rng.standard_normal((B_DEC, 192)).astype(np.float32))


def ensemble_reference(members, wts, fm, im, W, max_steps):
    """Beam search over the members' mean distribution from oracle.decoder_ref pieces: every member steps on the shared ids
    and is re-ordered by the shared parents; the step distribution and the selection are the float64 reference above.
    -> step_ids, parent_ids, scores [T,B,W], lengths, margin (the smallest rank-gap margin over all steps)."""
    B = fm.shape[0]
    cfg0 = members[0][1]
    V = cfg0.softmax_size
    st = []
    for p, cfg in members:
        keys, values = dr.memory_projections(p, cfg, np.repeat(fm, W, axis=0))
        c, h, _ = dr.rnn_init(p, cfg, np.repeat(im, W, axis=0), None)
        st.append(dict(keys=keys, values=values, c=c, h=h, att=np.zeros((B * W, cfg.attn_size), np.float32)))
    log_probs = np.full((B, W), -np.inf, np.float64)
    log_probs[:, 0] = 0
    finished = np.ones((B, W), np.int32)
    finished[:, 0] = 0
    lengths = np.zeros((B, W), np.int64)
    ids = np.full(B * W, cfg0.start_id, np.int64)
    out = dict(step_ids=[], parent_ids=[], scores=[])
    margin = np.inf
    for t in range(max_steps):
        logits = []
        for (p, cfg), s in zip(members, st):
            y, s['c'], s['h'], s['att'], _, _ = dr.decoder_step(p, cfg, s['keys'], s['values'], dr.embed(p['emb'], ids),
                                                                s['c'], s['h'], s['att'], None)
            logits.append((y @ p['W_o'] + p['b_o']).reshape(B, W, V))
        r = ref_select(ref_step_lp(np.stack(logits), wts), log_probs, finished, lengths, cfg0.end_id, 0.0)
        margin = min(margin, r['margin'])
        log_probs, finished, lengths = r['log_probs'], r['finished'], r['lengths']
        gidx = (np.arange(B)[:, None] * W + r['parent']).reshape(-1)
        for s in st:
            s['c'], s['h'], s['att'] = s['c'][gidx], s['h'][gidx], s['att'][gidx]
        out['step_ids'].append(r['word']); out['parent_ids'].append(r['parent']); out['scores'].append(r['scores'])
        ids = r['word'].reshape(-1).astype(np.int64)
        if finished.all():
            break
    res = {k: np.stack(v) for k, v in out.items()}
    res.update(lengths=lengths, margin=float(margin))
    return res


@functools.lru_cache(maxsize=None)
def mixed_members(eos_bias):
    out = []
    for k, kw in enumerate(MIXED_KW):
        spec, cfg = _spec_and_cfg(**kw)
        out.append((spec, cfg, _rand_params(cfg, MIXED_SEED + k, eos_bias)))
    return out


@functools.lru_cache(maxsize=None)
def mixed_reference(eos_bias):
    fm, im = _features()
    wts = np.asarray(MIXED_WEIGHTS, np.float32)
    return ensemble_reference([(p, cfg) for _, cfg, p in mixed_members(eos_bias)], wts, fm, im, W_DEC, MAX_STEPS)


def test_three_copies_match_the_single_decoder():
    """(a) three copies of one member, uniform weights: the mean of three equal distributions is that distribution."""
    spec, cfg = _spec_and_cfg()
    p = _rand_params(cfg, 5, EOS_BIAS)
    fm, im = _features()
    dec = cdec.Decoder(spec, p, DEV)
    single = dec.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, want_attention=False)
    ens = cdec.EnsembleDecoder([dec, dec, dec])
    res = ens.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS)
    for k in ('predicted_ids', 'parent_ids', 'lengths'):
        np.testing.assert_array_equal(res[k], single[k], err_msg=k)
    fin = np.isfinite(single['scores'])
    assert_close(np.where(fin, res['scores'], 0), np.where(fin, single['scores'], 0), 1e-5, 'scores')


def test_mixed_members_match_the_reference_loop():
    """(b) two LSTM members with different seeds and head counts plus an LN_LSTM member (the per-step launch chain) against
    the reference loop; (c) the graph replay (third call) is bit-identical to the eager first call."""
    ref = mixed_reference(EOS_BIAS)
    print('reference rank-gap margin over %d steps: %.2f (must exceed 1)' % (ref['step_ids'].shape[0], ref['margin']))
    assert ref['margin'] > 1.0, 'the seed cuts an entry short: a step of the float64 reference has a rank gap below the bar'
    fm, im = _features()
    ens = cdec.EnsembleDecoder([cdec.Decoder(spec, p, DEV) for spec, _, p in mixed_members(EOS_BIAS)], MIXED_WEIGHTS)
    eager = ens.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, use_graph=False, want_attention=True)
    assert eager['step_ids'].shape[0] == ref['step_ids'].shape[0]              # steps_executed
    np.testing.assert_array_equal(eager['step_ids'], ref['step_ids'])
    np.testing.assert_array_equal(eager['parent_ids'], ref['parent_ids'])
    np.testing.assert_array_equal(eager['lengths'], ref['lengths'])
    fin = np.isfinite(ref['scores'])
    assert_close(np.where(fin, eager['scores'], 0), np.where(fin, ref['scores'], 0), F32_RTOL, 'scores')
    assert eager['attn_hist'].shape == (eager['step_ids'].shape[0], B_DEC * W_DEC, 8 * 25)     # member 0's alignments
    ens.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS)                        # captures
    replay = ens.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, want_attention=True)
    assert next(iter(ens._ctxs.values())).graph is not None
    for k in ('step_ids', 'parent_ids', 'predicted_ids', 'lengths', 'scores', 'attn_hist'):
        np.testing.assert_array_equal(replay[k], eager[k], err_msg='replay: ' + k)


def test_rows_past_steps_executed_keep_their_poison():
    """(d) a strong EOS bias ends the loop early on the device: the executed prefix is the reference's and the rows of
    step_ids / parent_ids behind it are never written -- with a member on the per-step launch chain in the ensemble, whose
    state re-ordering must not index through those rows either."""
    ref = mixed_reference(EOS_BIAS_EARLY)
    assert ref['margin'] > 1.0
    T = ref['step_ids'].shape[0]
    assert T < MAX_STEPS, 'the early-exit case did not exit early'
    fm, im = _features()
    ens = cdec.EnsembleDecoder([cdec.Decoder(spec, p, DEV) for spec, _, p in mixed_members(EOS_BIAS_EARLY)], MIXED_WEIGHTS)
    for _ in range(3):                                                         # eager, captured, replayed
        res = ens.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS)
        assert res['step_ids'].shape[0] == T
        np.testing.assert_array_equal(res['step_ids'], ref['step_ids'])
        np.testing.assert_array_equal(res['parent_ids'], ref['parent_ids'])
        ctx = next(iter(ens._ctxs.values()))
        assert bool((ctx.step_ids[T:] == POISON).all()) and bool((ctx.parent_ids[T:] == POISON).all())


def test_streaming_lstm_members_match_the_single_decoder():
    """More than 32 rows: the members' LSTM step is the streaming kernel, as in Decoder.beam_search at that size."""
    spec, cfg = _spec_and_cfg()
    p = _rand_params(cfg, 9, EOS_BIAS)
    rng = np.random.default_rng(23)
    fm = rng.standard_normal((12, 25, 192)).astype(np.float32)
    im = rng.standard_normal((12, 192)).astype(np.float32)
    dec = cdec.Decoder(spec, p, DEV)
    single = dec.beam_search(dev(fm), dev(im), 3, 8, want_attention=False)
    res = cdec.EnsembleDecoder([dec, dec]).beam_search(dev(fm), dev(im), 3, 8)
    for k in ('predicted_ids', 'parent_ids', 'lengths'):
        np.testing.assert_array_equal(res[k], single[k], err_msg=k)
    fin = np.isfinite(single['scores'])
    assert_close(np.where(fin, res['scores'], 0), np.where(fin, single['scores'], 0), 1e-5, 'scores')


def test_named_entries_and_the_options_entry_decode_the_same_bits():
    """The frozen per-option entries forward to comic_decoder_beam_search, which is what beam_search calls: on one context,
    the named C entry and then beam_search with the same option leave the same step_ids, parent_ids, scores and lengths up
    to steps_executed, to the bit, and the context's workspace is the named query's.  V = 258 takes the one-workgroup
    step; V = 2304 (W * V = 9216 >= 8192, 2 chunks) the split step.  Both sides run the one loop, so this guards the
    forwarding, the argument order and the record Python builds, no more: that the loop still computes the bits it did
    is shown by tools/beam_digest.py on the two builds (profiles/r16_beam_digest_*.txt) and, for the workspace, by
    tests/golden/beam_workspace_sizes.json."""
    lib = L.load()
    B, W, steps = 2, 4, 6
    smp = cdec.BeamSampling(0.8, 3)
    rqd = cdec.BeamRequired(np.array([[[7]], [[9]]], np.int32))                # 1 word, stride 1: 2 banks
    cases = (('diverse', dict(groups=cdec.BeamGroups(2, 0.5)), lambda c: (None, C.byref(c.grp))),
             ('sampled', dict(sampling=smp), lambda c: (None, C.byref(c.smp))),
             ('truncated', dict(sampling=smp, truncation=cdec.BeamTruncation(top_k=5)),
              lambda c: (None, C.byref(c.smp), C.byref(c.trc))),
             ('required', dict(required=rqd), lambda c: (None, None, None, C.byref(c.rqd), c.req.data_ptr())))
    fm, im = (dev(a[:B]) for a in _features())
    for V in (258, 2304):
        spec, cfg = _spec_and_cfg(V=V)
        ens = cdec.EnsembleDecoder([cdec.Decoder(spec, _rand_params(cfg, 5, EOS_BIAS), DEV)])
        for name, kw, option_args in cases:
            opts = cdec.BeamOptions(**kw)
            ctx = ens._ctx(B, W, steps, [(fm, im)], opts)
            assert ctx.nbytes == getattr(lib, 'comic_decoder_beam_%s_workspace' % name)(ctx.descs, 1, B * W, steps, 0), (V, name)
            if opts.smp is not None:
                ctx.seed.copy_(torch.from_numpy(smp.seed_words(0)))
            if opts.required is not None:
                ctx.req.copy_(torch.from_numpy(rqd.ids))
            L.check(getattr(lib, 'comic_decoder_beam_' + name)(
                ctx.descs, ctx.ptabs, ctx.fm_ptrs, ctx.im_ptrs, ctx.wts, 1, B, W, steps, *option_args(ctx),
                ctx.step_ids.data_ptr(), ctx.parent_ids.data_ptr(), ctx.scores.data_ptr(), ctx.lengths.data_ptr(),
                ctx.finished.data_ptr(), ctx.hist_ptrs, ctx.steps.data_ptr(), ctx.ws.data_ptr(), ctx.nbytes, stream()), name)
            T = int(ctx.steps.item())
            named = dict(step_ids=ctx.step_ids[:T].cpu().numpy(), parent_ids=ctx.parent_ids[:T].cpu().numpy(),
                         scores=ctx.scores[:T].cpu().numpy(), lengths=ctx.lengths.cpu().numpy())
            res = ens.beam_search(fm, im, W, steps, use_graph=False, **kw)
            assert ens._ctx(B, W, steps, [(fm, im)], opts) is ctx              # (the decode ran on that very context)
            assert res['step_ids'].shape[0] == T, (V, name)
            for k, a in named.items():
                np.testing.assert_array_equal(res[k].view(np.int32 if a.itemsize == 4 else np.int64),
                                              a.view(np.int32 if a.itemsize == 4 else np.int64), err_msg='%d %s %s' % (V, name, k))


def _run(module_path, argv):
    import importlib.util
    spec = importlib.util.spec_from_file_location('cli_' + os.path.basename(module_path)[:-3], module_path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(argv)


def test_infer_cli_ensemble_of_one_checkpoint_twice(tmp_path):
    """(e) infer.py --infer_ensemble with one checkpoint listed twice writes captions___ens_N+N.json, equal to that
    checkpoint's own captions___N.json."""
    from tests import tiny_dataset
    ds = tiny_dataset.make(str(tmp_path / 'mscoco'), n_train=8, n_valid=4, n_test=4)
    logs = str(tmp_path / 'experiments')
    _run(os.path.join(ROOT, 'src', 'train.py'),
         ['--dataset_dir', ds, '--log_root', logs, '--cnn_name', 'inception_v3', '--cnn_fm_attention', 'Mixed_7c',
          '--cnn_input_size', '139,139', '--batch_size_eval', '4', '--rnn_size', '128', '--rnn_word_size', '64',
          '--train_mode', 'decoder', '--batch_size_train', '8', '--max_epoch', '1'])
    run_dir = os.path.join(logs, 'mscoco', 'radix_b256_add_LN_softmax_h8_tie_lstm_run_01')
    ckpts = sorted(glob.glob(os.path.join(run_dir, 'model_compact-*.npz')))
    assert ckpts, os.listdir(run_dir)
    num = os.path.basename(ckpts[-1])[len('model_compact-'):-len('.npz')]
    common = ['--infer_checkpoints_dir', run_dir, '--dataset_dir', ds, '--infer_set', 'test', '--batch_size_infer', '2',
              '--get_metric_score', '']
    _run(os.path.join(ROOT, 'src', 'infer.py'), common + ['--infer_checkpoints', num])
    _run(os.path.join(ROOT, 'src', 'infer.py'), common + ['--infer_checkpoints', '%s,%s' % (num, num), '--infer_ensemble'])
    out_dir = os.path.join(run_dir, 'infer_test_beam_3_lpen_0.0')
    own = json.load(open(os.path.join(out_dir, 'captions___%s.json' % num)))
    ens = json.load(open(os.path.join(out_dir, 'captions___ens_%s+%s.json' % (num, num))))
    assert len(ens) == 4 and ens == own
    assert len(open(os.path.join(out_dir, 'infer_speed.txt')).read().strip().splitlines()) >= 6      # header + two runs
