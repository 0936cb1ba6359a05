"""Constrained beam search on the GPU: the ban kernel (comic_beam_bans) against the plain-Python rule, the constrained step
(comic_beam_step_constrained) against float64, the whole decoder (Decoder / EnsembleDecoder .beam_search(constraints=))
against the reference loop of tests/beam_constraints_ref.py, the model level and `infer.py`'s flags on the tiny dataset.

Ids are compared exactly under the rule of tests/test_gpu_ensemble.py: every case asserts that its float64 reference
separates the ranks 1 ... W + 1 by more than the bar (margin > 1) in EVERY entry; no entry is excused.  The margins quoted in
the tests were computed on the CPU with this reference."""
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
from comic_amd.decoder import BeamConstraints
from tests import beam_constraints_ref as bref
from tests.gpu_util import DEV, F32_RTOL, assert_close, dev, stream, sync
from tests.test_gpu_ensemble import (POISON, STEP_CASES, _features, _rand_params, _run, _spec_and_cfg, ref_select, ref_step_lp,
                                     run_step, step_case)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_STEPS = 14


# ------------------------------------------------------------------ 1. the ban kernel ------------------------------------
ALPHABET = np.array([1, 2, 3, 5], np.int32)          # histories over four tokens: repeats occur
NGRAMS = [(0, 1), (1, 1), (2, 1), (3, 1), (4, 2)]    # (n, stride)


def _bans_state(B, W, V, t, finished_value=None):
    """The state step t - 1 left behind: histories of t - 1 tokens in buffer (t - 1) & 1, that step's words and parents (a
    rotation of the beams with one parent duplicated: no identity, two rows share a parent), lengths on both sides of
    min_length = 7, and at least one finished row."""
    rng = np.random.default_rng(1000 * V + 10 * t + W)
    R = B * W
    hist = np.full((2, R, MAX_STEPS), POISON, np.int32)
    prev = [[int(x) for x in rng.choice(ALPHABET, max(t - 1, 0))] for _ in range(R)]
    words = parents = None
    hists = [[] for _ in range(R)]
    if t > 0:
        for r in range(R):
            hist[(t - 1) & 1, r, :t - 1] = prev[r]
        parents = np.tile(np.roll(np.arange(W, dtype=np.int32), 1), (B, 1))
        if W > 1:
            parents[:, 0] = parents[:, 1]
        words = rng.choice(ALPHABET, (B, W)).astype(np.int32)
        hists = [prev[(r // W) * W + int(parents.reshape(-1)[r])] + [int(words.reshape(-1)[r])] for r in range(R)]
    finished = np.zeros(R, np.int32)
    if finished_value is not None:
        finished[:] = finished_value
    else:
        finished[R - 1] = 1
    lengths = rng.integers(0, MAX_STEPS, R).astype(np.int64)
    return dict(hist=hist, words=words, parents=parents, hists=hists, finished=finished, lengths=lengths)


def _run_bans(s, B, W, V, t, end_id, cons):
    lib = L.load()
    R, words = B * W, (V + 31) // 32
    d_hist = dev(s['hist'])
    d_bits = torch.full((R, words), -1, dtype=torch.int32, device=DEV)          # every word must be written
    d_words = dev(s['words']) if t > 0 else None
    d_parents = dev(s['parents']) if t > 0 else None
    d_fin, d_len = dev(s['finished']), dev(s['lengths'])
    cs = cons.c_struct()
    L.check(lib.comic_beam_bans(L.ptr(d_words), L.ptr(d_parents), d_fin.data_ptr(), d_len.data_ptr(), d_hist.data_ptr(),
                                d_bits.data_ptr(), t, B, W, V, MAX_STEPS, end_id, C.byref(cs), stream()), 'beam_bans')
    sync()
    return d_bits.cpu().numpy().view(np.uint32), d_hist.cpu().numpy()


@pytest.mark.parametrize('t', [0, 1, MAX_STEPS - 1])
@pytest.mark.parametrize('shape', [(1, 1, 33), (3, 3, 258), (2, 5, 9001)])       # V = 33: two words, the last partly used
def test_bans_kernel_matches_the_rule(shape, t):
    B, W, V = shape
    R, end_id = B * W, V - 1
    states = [_bans_state(B, W, V, t)] if R > 1 else [_bans_state(B, W, V, t, 0), _bans_state(B, W, V, t, 1)]
    rng = np.random.default_rng(5)
    for s in states:
        assert R == 1 or (s['finished'].any() and not s['finished'].all())
        for n, stride in NGRAMS:
            for K in (0, 2, 32):
                sup = tuple(int(x) for x in rng.choice(V - 1, K, replace=False))        # never end_id = V - 1
                kw = dict(min_length=7, no_repeat_ngram=n, ngram_stride=stride, suppress=sup)
                bits, hist = _run_bans(s, B, W, V, t, end_id, BeamConstraints(**kw))
                mask = bref.ban_mask(s['hists'], s['finished'], s['lengths'], V, end_id, **kw)
                np.testing.assert_array_equal(bits, bref.pack_bits(mask), err_msg='bits, n %d stride %d K %d' % (n, stride, K))
                assert not bits[s['finished'] != 0].any(), 'a finished row bans nothing'
                want = s['hist'].copy()
                for r in range(R):
                    want[t & 1, r, :t] = s['hists'][r]
                np.testing.assert_array_equal(hist, want, err_msg='history buffers')
    # the state bites: with n = 1 at the last step a live row bans tokens of its history, and min_length = 7 splits the rows
    if t == MAX_STEPS - 1:
        s = states[0]
        m = bref.ban_mask(s['hists'], s['finished'], s['lengths'], V, end_id, no_repeat_ngram=1)
        assert m[:, ALPHABET].any()
    if R > 1:
        assert (states[0]['lengths'] < 7).any() and (states[0]['lengths'] >= 7).any()


def test_bans_kernel_refuses_bad_constraints():
    lib = L.load()
    buf = torch.zeros(4096, dtype=torch.int32, device=DEV)

    def call(cons, V=258, end_id=257, t=0):
        cs = cons.c_struct()
        return lib.comic_beam_bans(None, None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), t, 1, 1, V,
                                   MAX_STEPS, end_id, C.byref(cs), stream())
    for cons, kw, what in ((BeamConstraints(no_repeat_ngram=3, ngram_stride=2), {}, 'ngram_stride'),
                           (BeamConstraints(suppress=(257,)), {}, 'end_id'),
                           (BeamConstraints(suppress=(300,)), {}, 'outside the vocabulary'),
                           (BeamConstraints(min_length=-1), {}, 'min_length'),
                           (BeamConstraints(), dict(V=70000, end_id=1), 'mask words'),
                           (BeamConstraints(), dict(t=1), 'needs the words')):
        assert call(cons, **kw) != 0
        assert what in lib.comic_last_error().decode(), (what, lib.comic_last_error())
    cs = BeamConstraints().c_struct()
    cs.n_suppress = 33
    assert lib.comic_beam_bans(None, None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 0, 1, 1, 258,
                               MAX_STEPS, 257, C.byref(cs), stream()) != 0
    assert 'n_suppress' in lib.comic_last_error().decode()
    sync()


# ------------------------------------------------------------------ 2. / 3. the constrained step -------------------------
def run_step_constrained(logits, wts, log_probs, finished, lengths, end_id, lpw, bits):
    lib = L.load()
    n, B, W, V = logits.shape
    d_lg, d_lp, d_fin, d_len = dev(logits), dev(log_probs), dev(finished), dev(lengths)
    d_bits = dev(np.ascontiguousarray(bits).view(np.int32))
    word = torch.full((B, W), -1, dtype=torch.int32, device=DEV)
    parent = torch.full((B, W), -1, dtype=torch.int32, device=DEV)
    scores = torch.zeros((B, W), dtype=torch.float32, device=DEV)
    nbytes = int(lib.comic_beam_step_ensemble_workspace(n, B, W, V))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    wt = (C.c_float * n)(*[float(w) for w in wts])
    L.check(lib.comic_beam_step_constrained(d_lg.data_ptr(), wt, n, d_lp.data_ptr(), d_fin.data_ptr(), d_len.data_ptr(),
                                            word.data_ptr(), parent.data_ptr(), scores.data_ptr(), B, W, V, end_id,
                                            float(lpw), d_bits.data_ptr(), (V + 31) // 32, ws.data_ptr(), nbytes, stream()),
            'beam_step_constrained')
    sync()
    return dict(word=word.cpu().numpy(), parent=parent.cpu().numpy(), scores=scores.cpu().numpy(),
                log_probs=d_lp.cpu().numpy(), finished=d_fin.cpu().numpy(), lengths=d_len.cpu().numpy(),
                split=int(lib.comic_beam_step_ensemble_path()))


@functools.lru_cache(maxsize=None)
def constrained_step_case(shape, state, lpw):
    """Half of all candidates banned, and with them every candidate the unconstrained reference selects: each case bites."""
    c = step_case(shape, state, lpw)
    n, B, W, V = shape
    mask = np.random.default_rng(1).random((B, W, V)) < 0.5
    mask[np.arange(B)[:, None], c['ref']['parent'], c['ref']['word']] = True
    live = c['finished'] == 0
    lp = np.where(mask & live[:, :, None], -np.inf, ref_step_lp(c['logits'], c['wts']))
    return c, mask, ref_select(lp, c['log_probs'], c['finished'], c['lengths'], c['end_id'], lpw)


def test_constrained_step_cases_meet_the_margin():
    """Checked on the CPU: the smallest margin over the 17 cases is 6.5."""
    margins = [constrained_step_case(*case)[2]['margin'] for case in STEP_CASES]
    print('rank-gap margins of the constrained step cases: min %.2f' % min(margins))
    assert len(STEP_CASES) == 17 and min(margins) > 6.0


@pytest.mark.parametrize('shape,state,lpw', STEP_CASES)
def test_constrained_step_matches_float64(shape, state, lpw):
    c, mask, ref = constrained_step_case(shape, state, lpw)
    print('reference rank-gap margin %.2f (must exceed 1)' % ref['margin'])
    assert ref['margin'] > 1.0
    un = c['ref']
    assert not (np.array_equal(ref['word'], un['word']) and np.array_equal(ref['parent'], un['parent'])), \
        'the mask does not change what the step selects'
    n, B, W, V = shape
    got = run_step_constrained(c['logits'], c['wts'], c['log_probs'], c['finished'], c['lengths'], c['end_id'], lpw,
                               bref.pack_bits(mask.reshape(B * W, V)))
    assert got['split'] == (1 if (V == 9001 and lpw == 0.0) else 0)            # the same rule as the unconstrained step
    for k in ('word', 'parent', 'finished', 'lengths'):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert_close(got['scores'], ref['scores'], F32_RTOL, 'scores')
    assert_close(got['log_probs'], ref['log_probs'], F32_RTOL, 'new log_probs')
    bidx = np.arange(B)[:, None]
    live_parent = c['finished'][bidx, got['parent']] == 0
    assert live_parent.any()
    assert not (mask[bidx, got['parent'], got['word']] & live_parent).any(), 'a banned candidate of a live beam was selected'


@pytest.mark.parametrize('shape', [(3, 3, 3, 258), (2, 2, 5, 9001)])
def test_all_zero_mask_is_the_ensemble_step_to_the_bit(shape):
    n, B, W, V = shape
    for state in ('init', 'mid'):
        c = step_case(shape, state, 0.0)
        args = (c['logits'], c['wts'], c['log_probs'], c['finished'], c['lengths'], c['end_id'], 0.0)
        plain = run_step(*args)
        zero = run_step_constrained(*args, np.zeros((B * W, (V + 31) // 32), np.uint32))
        for k in ('word', 'parent', 'finished', 'lengths', 'scores', 'log_probs', 'split'):
            np.testing.assert_array_equal(zero[k], plain[k], err_msg=k)


# ------------------------------------------------------------------ 4. - 8. the whole decoder ----------------------------
W_DEC = 3


def _check_decode(res, ref):
    assert res['step_ids'].shape[0] == ref['step_ids'].shape[0]                # steps_executed
    np.testing.assert_array_equal(res['step_ids'], ref['step_ids'])
    np.testing.assert_array_equal(res['parent_ids'], ref['parent_ids'])
    np.testing.assert_array_equal(res['lengths'], ref['lengths'])
    fin = np.isfinite(ref['scores'])
    assert_close(np.where(fin, res['scores'], 0), np.where(fin, ref['scores'], 0), F32_RTOL, 'scores')


def _differs(a, b):
    return a['step_ids'].shape != b['step_ids'].shape or not np.array_equal(a['step_ids'], b['step_ids'])


def _single(seed, fm, im, max_steps, **kw):
    spec, cfg = _spec_and_cfg()
    p = _rand_params(cfg, seed, 3.0)
    ref = bref.constrained_reference([(p, cfg)], np.ones(1, np.float32), fm, im, W_DEC, max_steps, **kw)
    return spec, cfg, p, ref


def test_single_decoder_all_three_constraints():
    """Checked on the CPU: 14 steps with finished and live beams side by side, margin 2.56; each of the three constraints
    matters (dropping any one changes the ids)."""
    kw = dict(no_repeat_ngram=2, min_length=6, suppress=(7, 155))
    fm, im = _features()
    spec, cfg, p, ref = _single(61, fm, im, MAX_STEPS, **kw)
    print('reference rank-gap margin over %d steps: %.2f (must exceed 1)' % (ref['step_ids'].shape[0], ref['margin']))
    assert ref['margin'] > 1.0 and ref['step_ids'].shape[0] == MAX_STEPS
    assert len(set(ref['lengths'].reshape(-1).tolist())) > 1 and ref['lengths'].min() < MAX_STEPS     # finished beside live
    for drop in (dict(no_repeat_ngram=0), dict(min_length=0), dict(suppress=())):
        other = bref.constrained_reference([(p, cfg)], np.ones(1, np.float32), fm, im, W_DEC, MAX_STEPS, **dict(kw, **drop))
        assert _differs(other, ref), 'dropping %r does not change the ids' % (drop,)
    dec = cdec.Decoder(spec, p, DEV)
    cons = BeamConstraints(**kw)
    eager = dec.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, want_attention=True, use_graph=False, constraints=cons)
    _check_decode(eager, ref)
    pred = eager['predicted_ids']                                              # [T, B, W]
    end = spec.end_id
    for b in range(pred.shape[1]):
        for w in range(W_DEC):
            seq = pred[:, b, w].tolist()
            assert 7 not in seq and 155 not in seq
            assert end not in seq[:6], 'a caption ends before min_length'
            body = seq[:seq.index(end)] if end in seq else seq
            grams = list(zip(body[:-1], body[1:]))
            assert len(grams) == len(set(grams)), 'a bigram repeats: %r' % (body,)
    dec.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, constraints=cons)      # captures
    replay = dec.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, want_attention=True, constraints=cons)
    ctxs = dec._self_ensemble._ctxs
    assert len(ctxs) == 1 and next(iter(ctxs.values())).graph is not None
    for k in ('step_ids', 'parent_ids', 'predicted_ids', 'lengths', 'scores', 'attn_hist'):
        np.testing.assert_array_equal(replay[k], eager[k], err_msg='replay: ' + k)


def test_early_exit_keeps_the_poison():
    """Checked on the CPU: the reference ends after 8 of 14 steps, margin 11.3.  The ban kernel of the steps behind the
    end returns at once like every launch of a step: rows past steps_executed are never written, eager or replayed."""
    kw = dict(no_repeat_ngram=2, min_length=6, suppress=(120, 151))
    fm, im = _features()
    spec, cfg, p, ref = _single(59, fm, im, MAX_STEPS, **kw)
    T = ref['step_ids'].shape[0]
    print('reference: %d steps, rank-gap margin %.2f' % (T, ref['margin']))
    assert ref['margin'] > 1.0 and T == 8
    dec = cdec.Decoder(spec, p, DEV)
    for _ in range(3):                                                         # eager, captured, replayed
        res = dec.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, want_attention=False, constraints=BeamConstraints(**kw))
        _check_decode(res, ref)
        ctx = next(iter(dec._self_ensemble._ctxs.values()))
        assert bool((ctx.step_ids[T:] == POISON).all()) and bool((ctx.parent_ids[T:] == POISON).all())
    assert ctx.graph is not None


def test_stride():
    """Checked on the CPU: 14 steps, margin 2.87; the ids differ from stride 1 and from no n-gram blocking."""
    kw = dict(no_repeat_ngram=2, ngram_stride=2, min_length=8)
    fm, im = _features()
    spec, cfg, p, ref = _single(108, fm, im, MAX_STEPS, **kw)
    print('reference rank-gap margin %.2f' % ref['margin'])
    assert ref['margin'] > 1.0 and ref['step_ids'].shape[0] == MAX_STEPS
    for other in (dict(kw, ngram_stride=1), dict(kw, no_repeat_ngram=0, ngram_stride=1)):
        assert _differs(bref.constrained_reference([(p, cfg)], np.ones(1, np.float32), fm, im, W_DEC, MAX_STEPS, **other), ref)
    res = cdec.Decoder(spec, p, DEV).beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, want_attention=False,
                                                 constraints=BeamConstraints(**kw))
    _check_decode(res, ref)


def test_ensemble():
    """Two members with different head counts, weights [0.6, 0.4].  Checked on the CPU: 14 steps, margin 3.96."""
    kw = dict(no_repeat_ngram=2, min_length=6)
    fm, im = _features()
    members = []
    for seed, geo in ((38, dict()), (39, dict(H=4))):
        spec, cfg = _spec_and_cfg(**geo)
        members.append((spec, cfg, _rand_params(cfg, seed, 3.0)))
    wts = [0.6, 0.4]
    ref = bref.constrained_reference([(p, cfg) for _, cfg, p in members], np.asarray(wts, np.float32), fm, im, W_DEC, MAX_STEPS,
                                     **kw)
    print('reference rank-gap margin %.2f' % ref['margin'])
    assert ref['margin'] > 1.0 and ref['step_ids'].shape[0] == MAX_STEPS
    ens = cdec.EnsembleDecoder([cdec.Decoder(spec, p, DEV) for spec, _, p in members], wts)
    _check_decode(ens.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, constraints=BeamConstraints(**kw)), ref)


def test_more_than_32_rows():
    """B = 12, W = 3: the members' LSTM step is the streaming kernel.  Checked on the CPU: 10 steps, margin 2.64."""
    kw = dict(no_repeat_ngram=2, min_length=4)
    rng = np.random.default_rng(23)
    fm = rng.standard_normal((12, 25, 192)).astype(np.float32)
    im = rng.standard_normal((12, 192)).astype(np.float32)
    spec, cfg, p, ref = _single(261, fm, im, 10, **kw)
    print('reference rank-gap margin %.2f' % ref['margin'])
    assert ref['margin'] > 1.0 and ref['step_ids'].shape[0] == 10
    res = cdec.Decoder(spec, p, DEV).beam_search(dev(fm), dev(im), W_DEC, 10, want_attention=False,
                                                 constraints=BeamConstraints(**kw))
    _check_decode(res, ref)


def test_refused_on_the_host_and_by_the_library():
    spec, cfg = _spec_and_cfg()
    dec = cdec.Decoder(spec, _rand_params(cfg, 61, 3.0), DEV)
    fm, im = _features()
    with pytest.raises(ValueError, match='min_length'):
        dec.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, constraints=BeamConstraints(min_length=MAX_STEPS))
    with pytest.raises(ValueError, match='too small'):
        dec.beam_search(dev(fm), dev(im), W_DEC, 258, constraints=BeamConstraints(min_length=2))
    assert '_self_ensemble' not in dec.__dict__                               # refused before anything was built


# ------------------------------------------------------------------ 9. no constraints, no change --------------------------
def test_none_and_inactive_constraints_change_nothing():
    spec, cfg = _spec_and_cfg()
    p = _rand_params(cfg, 5, 3.0)
    fm, im = _features()
    dec = cdec.Decoder(spec, p, DEV)
    ens = cdec.EnsembleDecoder([dec, dec])
    for run, kw in ((dec.beam_search, dict(want_attention=False)), (ens.beam_search, dict())):
        base = run(dev(fm), dev(im), W_DEC, MAX_STEPS, use_graph=False, **kw)
        for cons in (None, BeamConstraints()):
            res = run(dev(fm), dev(im), W_DEC, MAX_STEPS, use_graph=False, constraints=cons, **kw)
            assert sorted(res) == sorted(base)
            for k in base:
                np.testing.assert_array_equal(res[k], base[k], err_msg=k)
    plain_key = cdec.BeamOptions().ctx_key()                                      # the plain contexts only
    assert '_self_ensemble' not in dec.__dict__ and all(k[3] == plain_key for k in ens._ctxs)


# ------------------------------------------------------------------ 10. / 11. model and CLI --------------------------------
@pytest.fixture(scope='module')
def tiny_run(tmp_path_factory):
    """The tiny dataset and a one-epoch decoder-mode run on it (radix tokens)."""
    from tests import tiny_dataset
    tmp = tmp_path_factory.mktemp('constraints')
    ds = tiny_dataset.make(str(tmp / 'mscoco'), n_train=8, n_valid=4, n_test=4)
    logs = str(tmp / 'experiments')
    _run(os.path.join(ROOT, 'src', 'train.py'),
         ['--dataset_dir', ds, '--log_root', logs, '--cnn_name', 'inception_v3', '--cnn_fm_attention', 'Mixed_7c',
          '--cnn_input_size', '139,139', '--batch_size_eval', '4', '--rnn_size', '128', '--rnn_word_size', '64',
          '--train_mode', 'decoder', '--batch_size_train', '8', '--max_epoch', '1'])
    run_dir = os.path.join(logs, 'mscoco', 'radix_b256_add_LN_softmax_h8_tie_lstm_run_01')
    ckpts = sorted(glob.glob(os.path.join(run_dir, 'model_compact-*.npz')))
    assert ckpts, os.listdir(run_dir)
    return ds, run_dir, ckpts[-1]


def test_model_level_words_on_radix_tokens(tiny_run):
    """_decode_features with min_length = 3 and no_repeat_ngram = 1 in WORDS: in token space every top caption has at
    least 3 * word_len tokens before <EOS> and no aligned word twice.  (Nothing is asserted on the decoded text:
    id_to_caption skips word ids beyond the vocabulary.)"""
    import importlib.util
    from comic_amd import configuration as conf, inputs, model as mdl
    from comic_amd.ops import number_to_base
    ds, run_dir, ckpt = tiny_run
    sp = importlib.util.spec_from_file_location('cli_infer_constraints', os.path.join(ROOT, 'src', 'infer.py'))
    cli = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(cli)
    args = cli.create_parser().parse_args(['--infer_checkpoints_dir', run_dir, '--dataset_dir', ds, '--infer_set', 'test',
                                           '--batch_size_infer', '2', '--infer_min_length', '3', '--infer_no_repeat_ngram', '1'])
    c = conf.load_config(os.path.join(run_dir, 'config.pkl'))
    c.__dict__.update({k: v for k, v in args.__dict__.items() if v is not None})
    assert c.token_type == 'radix'
    mdl.reset_default_graph()
    man = inputs.InputManager(c, is_inference=True)                           # (reads the vocabulary into the configuration)
    try:
        c = man.config
        word_len = len(number_to_base(len(c.wtoi), c.radix_base))
        cons = cdec.constraints_from_config(c)
        assert cons == BeamConstraints(min_length=3 * word_len, no_repeat_ngram=word_len, ngram_stride=word_len)
        man.enable_device_preprocess(DEV)
        c.resume_training = False
        c.checkpoint_path = ckpt
        m = mdl.CaptionModel(c, mode='infer', batch_ops=man.batch_infer, reuse=False, name='inference', device=DEV)
        m.restore_model()
        im_embed, fm = m._next_infer_features()
        ids, _ = m._decode_features(im_embed, fm, 3, c.infer_max_length, top_beam=True, want_attention=False,
                                    options=cdec.BeamOptions(constraints=cons))
    finally:
        man.close()
        mdl.reset_default_graph()
    end = m.spec.end_id
    assert ids.shape[0] == 2
    for row in np.asarray(ids).tolist():
        body = row[:row.index(end)] if end in row else row
        assert len(body) >= 3 * word_len, body
        words = [tuple(body[i:i + word_len]) for i in range(0, len(body) - word_len + 1, word_len)]
        assert len(words) == len(set(words)), 'an aligned word repeats: %r' % (words,)


def test_infer_cli_flags_write_a_directory_of_their_own(tiny_run):
    ds, run_dir, ckpt = tiny_run
    num = os.path.basename(ckpt)[len('model_compact-'):-len('.npz')]
    common = ['--infer_checkpoints_dir', run_dir, '--dataset_dir', ds, '--infer_set', 'test', '--batch_size_infer', '2',
              '--get_metric_score', '', '--infer_checkpoints', num]
    infer = os.path.join(ROOT, 'src', 'infer.py')
    _run(infer, common + ['--infer_min_length', '3', '--infer_no_repeat_ngram', '1'])
    plain_dir = os.path.join(run_dir, 'infer_test_beam_3_lpen_0.0')
    cons_dir = plain_dir + '_min3_ngram1_sup0'
    assert not os.path.exists(plain_dir)
    caps = json.load(open(os.path.join(cons_dir, 'captions___%s.json' % num)))
    assert len(caps) == 4
    _run(infer, common)
    plain = json.load(open(os.path.join(plain_dir, 'captions___%s.json' % num)))
    assert len(plain) == 4 and sorted(os.listdir(cons_dir)) == sorted(os.listdir(plain_dir))
