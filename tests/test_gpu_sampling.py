"""Sampling inside the beam step on the GPU: the generator (comic_beam_sample_noise) and the sampled step
(comic_beam_step_sampled) against the float64 reference of tests/beam_sampling_ref.py, the whole decoder (Decoder /
EnsembleDecoder.beam_search(sampling=)) against the reference loop, and `infer.py`'s flags on the tiny dataset.

Ids are compared exactly under the rule of tests/test_gpu_ensemble.py, applied per slot: every case asserts that its float64
reference separates the best and second-best rank of EVERY live slot of EVERY entry by more than GAP * max(1, |rank|)
(margin > 1); no entry is excused.  The margins quoted below were computed on the CPU with this reference."""
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
from comic_amd.decoder import BeamConstraints, BeamGroups, BeamSampling
from tests import beam_constraints_ref as bref
from tests import beam_sampling_ref as sref
from tests.gpu_util import DEV, F32_RTOL, assert_close, dev, stream, sync
from tests.test_gpu_constraints import tiny_run  # noqa: F401  (the fixture: a one-epoch run on the tiny dataset)
from tests.test_gpu_ensemble import POISON, _features, _rand_params, _run, _spec_and_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_STEPS = 14
SEED = 5

# (n, B, W, V): smallest; radix vocabulary with three members; the split form on the register-resident chunk kernel; the
# split form on the rescanning one (5 columns x 9 slots = 45 > 40 register slots); more than 32 rows; the widest entry;
# the most members.  Smallest margin over all 28 cases (init / mid, temperature 1.0 / 0.7), computed on the CPU: 5.7.
SHAPES = [(1, 2, 3, 17), (3, 3, 4, 258), (2, 2, 5, 9001), (2, 2, 9, 9001), (1, 33, 2, 258), (1, 1, 64, 300), (8, 1, 2, 300)]
STEP_CASES = [(s, state, temp) for s in SHAPES for state in ('init', 'mid') for temp in (1.0, 0.7)]


def _seed_dev(seed, base):
    return torch.from_numpy(np.array([seed, base], np.uint64).view(np.int64)).to(DEV)


# ------------------------------------------------------------------ the generator ------------------------------------
@pytest.mark.parametrize('B,W,t,V', [(3, 4, 0, 258), (2, 64, 7, 9001)])
@pytest.mark.parametrize('base', [0, 1000])
def test_noise_matches_the_reference(B, W, t, V, base):
    """k to the bit; |g - g64| <= 1e-5: a 2-ulp logf leaves 2.4e-7 relative on -log u, i.e. 2.4e-7 absolute on g, plus 2 ulp
    of |g| <= 16.64, together 4.2e-6, taken with a factor two.  A native-approximation logf fails this near u -> 1."""
    lib = L.load()
    seed = _seed_dev(SEED, base)
    k = torch.full((B * W, V), -1, dtype=torch.int32, device=DEV)
    g = torch.zeros((B * W, V), dtype=torch.float32, device=DEV)
    L.check(lib.comic_beam_sample_noise(seed.data_ptr(), B, W, t, V, k.data_ptr(), g.data_ptr(), stream()), 'beam_sample_noise')
    sync()
    rk, _, rg = sref.noise(SEED, base, B, W, t, V)
    np.testing.assert_array_equal(k.cpu().numpy().reshape(B, W, V), rk)
    err = float(np.abs(g.cpu().numpy().reshape(B, W, V).astype(np.float64) - rg).max())
    print('max |g - g64| = %.3e (bound 1e-5)' % err)
    assert err <= 1e-5


# ------------------------------------------------------------------ the sampled step ---------------------------------
def run_step_sampled(logits, wts, log_probs, finished, lengths, end_id, temperature, seed=SEED, base=0, t=0, bits=None,
                     workspace=True):
    lib = L.load()
    n, B, W, V = logits.shape
    d_lg, d_lp, d_fin, d_len = dev(logits), dev(log_probs), dev(finished), dev(lengths)
    d_bits = dev(np.ascontiguousarray(bits).view(np.int32)) if bits is not None else None
    word = torch.full((B, W), -1, dtype=torch.int32, device=DEV)
    parent = torch.full((B, W), -1, dtype=torch.int32, device=DEV)
    scores = torch.zeros((B, W), dtype=torch.float32, device=DEV)
    nbytes = int(lib.comic_beam_step_sampled_workspace(n, B, W, V))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ws_ptr, ws_bytes = (ws.data_ptr(), nbytes) if workspace else (None, 0)
    wt = (C.c_float * n)(*[float(w) for w in wts])
    d_seed = _seed_dev(seed, base)
    smp = BeamSampling(temperature, seed).c_struct(d_seed.data_ptr())
    L.check(lib.comic_beam_step_sampled(d_lg.data_ptr(), wt, n, d_lp.data_ptr(), d_fin.data_ptr(), d_len.data_ptr(),
                                        word.data_ptr(), parent.data_ptr(), scores.data_ptr(), B, W, V, end_id,
                                        L.ptr(d_bits), (V + 31) // 32, C.byref(smp), t, ws_ptr, ws_bytes, stream()),
            'beam_step_sampled')
    sync()
    return dict(word=word.cpu().numpy(), parent=parent.cpu().numpy(), scores=scores.cpu().numpy(),
                log_probs=d_lp.cpu().numpy(), finished=d_fin.cpu().numpy(), lengths=d_len.cpu().numpy(),
                split=int(lib.comic_beam_step_ensemble_path()))


def _state(c):
    return c['logits'], c['wts'], c['log_probs'], c['finished'], c['lengths'], c['end_id']


def _check_step(got, ref):
    for k in ('word', 'finished', 'lengths'):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    W = got['parent'].shape[1]
    np.testing.assert_array_equal(got['parent'], np.tile(np.arange(W, dtype=np.int32), (got['parent'].shape[0], 1)), 'parent')
    np.testing.assert_array_equal(got['scores'], got['log_probs'], 'scores are the state')
    assert_close(got['scores'], ref['scores'], F32_RTOL, 'scores')
    assert_close(got['log_probs'], ref['log_probs'], F32_RTOL, 'new log_probs')


def _noise_decides(c, ref):
    """The share of live slots whose choice differs from that of a step without noise."""
    live = c['finished'] == 0
    return float((ref['word'] != ref['greedy'])[live].mean())


@pytest.mark.parametrize('shape,state,temp', STEP_CASES)
def test_sampled_step_matches_float64(shape, state, temp):
    """Noise seed 5, base 0, t 0.  A kernel that ignored the noise fails: in every case some live slot leaves the greedy
    choice, and in every case but the smallest, V = 17 -- whose six (init) or four (mid) live slots keep the mode too often:
    the share is 0.5 and 0.25 there, computed on the CPU -- more than half of the live slots do."""
    c = sref.sampled_case(shape, state, temp, SEED, 0, 0)
    ref = c['ref']
    share = _noise_decides(c, ref)
    print('reference rank-gap margin %.2f (must exceed 1); %.2f of the live slots leave the greedy choice' % (ref['margin'], share))
    assert ref['margin'] > 1.0, 'the seed of this case does not separate the ranks of the float64 reference'
    assert share > 0.0 and (share > 0.5 or shape[3] == 17), 'the noise does not change what the step selects'
    got = run_step_sampled(*_state(c), temp)
    # the split form runs exactly where the rule of the plain step says, on the entry-wide W * V
    assert got['split'] == (1 if shape[3] == 9001 else 0)
    _check_step(got, ref)


def test_sampled_step_peaked_logits():
    """Three members whose rows each have one dominant entry: the step distribution is log w_m at three tokens and below
    -25 elsewhere, the noise decides between the three; scores and ids against the float64 reference as in the sibling"""
    shape, temp = (3, 3, 4, 258), 0.7
    c = sref.peaked_inputs(shape)
    g = sref.noise(SEED, 0, shape[1], shape[2], 0, shape[3])[2]
    ref = sref.ref_select_sampled(c['lp'], c['log_probs'], c['finished'], c['lengths'], c['end_id'], g, sref.inv_temp_of(temp))
    share = _noise_decides(c, ref)
    print('peaked: reference rank-gap margin %.2f (must exceed 1); %.2f of the live slots leave the greedy choice' % (ref['margin'], share))
    assert ref['margin'] > 1.0
    assert np.abs(c['logits']).max() > 250
    _check_step(run_step_sampled(*_state(c), temp), ref)


def test_other_seed_words_and_step():
    """Seed 5, base 1000, t 3: checked on the CPU, the smallest margin over the 28 cases is 16; here the two split shapes
    and the radix one."""
    for shape in ((3, 3, 4, 258), (2, 2, 5, 9001), (2, 2, 9, 9001)):
        c = sref.sampled_case(shape, 'mid', 0.7, SEED, 1000, 3)
        assert c['ref']['margin'] > 1.0
        assert not np.array_equal(c['ref']['word'], sref.sampled_case(shape, 'mid', 0.7, SEED, 0, 0)['ref']['word'])
        _check_step(run_step_sampled(*_state(c), 0.7, base=1000, t=3), c['ref'])


# ------------------------------------------------------------------ step properties ------------------------------------
@pytest.mark.parametrize('shape', [(3, 3, 4, 258), (2, 2, 5, 9001), (2, 2, 9, 9001)])
def test_same_seed_same_bits_other_seed_other_ids(shape):
    """Seed 6 (margin over the 28 cases on the CPU: 6.4) gives other ids, and they are the reference's."""
    c = sref.sampled_case(shape, 'mid', 0.7)
    a = run_step_sampled(*_state(c), 0.7)
    b = run_step_sampled(*_state(c), 0.7)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    c6 = sref.sampled_case(shape, 'mid', 0.7, 6)
    assert c6['ref']['margin'] > 1.0
    assert not np.array_equal(c6['ref']['word'], c['ref']['word'])
    _check_step(run_step_sampled(*_state(c6), 0.7, seed=6), c6['ref'])


@pytest.mark.parametrize('shape', [(3, 3, 4, 258), (2, 2, 5, 9001), (2, 2, 9, 9001)])
def test_with_and_without_a_workspace(shape):
    for state in ('init', 'mid'):
        c = sref.sampled_case(shape, state, 0.7)
        assert c['ref']['margin'] > 1.0
        with_ws = run_step_sampled(*_state(c), 0.7)
        without = run_step_sampled(*_state(c), 0.7, workspace=False)
        assert with_ws['split'] == (1 if shape[3] == 9001 else 0) and without['split'] == 0
        for k in ('word', 'parent', 'finished', 'lengths'):
            np.testing.assert_array_equal(with_ws[k], without[k], err_msg=k)
        _check_step(without, c['ref'])


@functools.lru_cache(maxsize=None)
def banned_case(shape, state, temp):
    """Half of all candidates banned, and with them every candidate the unbanned sampled reference selects."""
    c = sref.sampled_case(shape, state, temp)
    n, B, W, V = shape
    mask = np.random.default_rng(1).random((B, W, V)) < 0.5
    mask[np.arange(B)[:, None], c['ref']['parent'], c['ref']['word']] = True
    live = c['finished'] == 0
    lp = np.where(mask & live[:, :, None], -np.inf, c['lp'])
    g = sref.noise(SEED, 0, B, W, 0, V)[2]
    return c, mask, sref.ref_select_sampled(lp, c['log_probs'], c['finished'], c['lengths'], c['end_id'], g,
                                            sref.inv_temp_of(temp))


@pytest.mark.parametrize('shape,state,temp', [((3, 3, 4, 258), 'mid', 0.7), ((2, 2, 5, 9001), 'init', 0.7),
                                              ((2, 2, 9, 9001), 'mid', 1.0)])
def test_sampled_step_under_a_ban_mask(shape, state, temp):
    """Checked on the CPU: margins 761, 21.5 and 11.0 (the rescanning shape at temperature 0.7 has a reference margin of
    0.87 under this mask, so that case runs at 1.0)."""
    c, mask, ref = banned_case(shape, state, temp)
    print('reference rank-gap margin %.2f (must exceed 1)' % ref['margin'])
    assert ref['margin'] > 1.0
    live = c['finished'] == 0
    assert (ref['word'] != c['ref']['word'])[live].all(), 'the mask does not change what the step selects'
    n, B, W, V = shape
    got = run_step_sampled(*_state(c), temp, bits=bref.pack_bits(mask.reshape(B * W, V)))
    assert got['split'] == (1 if V == 9001 else 0)
    _check_step(got, ref)
    bidx = np.arange(B)[:, None]
    assert not (mask[bidx, got['parent'], got['word']] & live).any(), 'a banned candidate of a live slot was selected'


@pytest.mark.parametrize('shape', [(3, 3, 4, 258), (2, 2, 5, 9001)])
def test_all_zero_mask_is_no_mask_to_the_bit(shape):
    n, B, W, V = shape
    for state in ('init', 'mid'):
        c = sref.sampled_inputs(shape, state)
        none = run_step_sampled(*_state(c), 0.7)
        zero = run_step_sampled(*_state(c), 0.7, bits=np.zeros((B * W, (V + 31) // 32), np.uint32))
        for k in ('word', 'parent', 'finished', 'lengths', 'scores', 'log_probs', 'split'):
            np.testing.assert_array_equal(zero[k], none[k], err_msg=k)


def test_step_refuses():
    lib = L.load()
    B, W, V = 1, 4, 17
    buf = torch.zeros(4096, dtype=torch.int32, device=DEV)
    wt = (C.c_float * 1)(1.0)
    p = buf.data_ptr()

    def call(smp, W=W):
        return lib.comic_beam_step_sampled(p, wt, 1, p, p, p, p, p, p, B, W, V, V - 1, None, 0,
                                           C.byref(smp) if smp is not None else None, 0, None, 0, stream())
    for smp, kw, what in ((None, {}, 'null sampling'),
                          (L.BeamSampling(1.0, None), {}, 'null seed_dev'),
                          (L.BeamSampling(0.0, p), {}, 'temperature'),
                          (L.BeamSampling(-1.0, p), {}, 'temperature'),
                          (L.BeamSampling(float('nan'), p), {}, 'temperature'),
                          (L.BeamSampling(float('inf'), p), {}, 'temperature'),
                          (L.BeamSampling(1e-39, p), {}, 'reciprocal'),
                          (L.BeamSampling(1.0, p), dict(W=0), 'number of samples'),
                          (L.BeamSampling(1.0, p), dict(W=65), 'number of samples')):
        assert call(smp, **kw) != 0
        assert what in lib.comic_last_error().decode(), (what, lib.comic_last_error())
    assert lib.comic_beam_sample_noise(None, 1, 1, 0, 17, p, p, stream()) != 0
    assert 'null seed_dev' in lib.comic_last_error().decode()
    sync()


# ------------------------------------------------------------------ the whole decoder ------------------------------------
N_DEC, TEMP = 4, 0.8


def _check_decode(res, ref):
    assert res['step_ids'].shape[0] == ref['step_ids'].shape[0]                # steps_executed
    np.testing.assert_array_equal(res['step_ids'], ref['step_ids'])
    np.testing.assert_array_equal(res['parent_ids'], ref['parent_ids'])
    np.testing.assert_array_equal(res['lengths'], ref['lengths'])
    assert_close(res['scores'], ref['scores'], F32_RTOL, 'scores')
    assert res['groups'] == 1
    assert_close(res['log_probs'], ref['log_probs'], F32_RTOL, 'final log_probs')


@functools.lru_cache(maxsize=None)
def _single(pseed, eos_bias, nseed, **cons):
    fm, im = _features()
    spec, cfg = _spec_and_cfg()
    p = _rand_params(cfg, pseed, eos_bias)
    ref = sref.sampled_reference([(p, cfg)], np.ones(1, np.float32), fm, im, N_DEC, MAX_STEPS, nseed, TEMP, **cons)
    return spec, cfg, p, ref


def test_single_decoder_four_samples_and_a_new_seed_on_replay():
    """n = 4 at temperature 0.8.  Checked on the CPU: noise seed 2 runs 14 steps with finished and live chains side by
    side, margin 178.7; seed 3 likewise, margin 158.1, other ids.  Eager, capture, replay; then seed 3 on the SAME captured
    graph: the seed words live in device memory."""
    fm, im = _features()
    spec, cfg, p, ref = _single(61, 3.0, 2)
    ref3 = _single(61, 3.0, 3)[3]
    print('reference rank-gap margins over %d steps: %.2f, %.2f (must exceed 1)' % (ref['step_ids'].shape[0], ref['margin'],
                                                                                     ref3['margin']))
    assert ref['margin'] > 1.0 and ref3['margin'] > 1.0 and ref['step_ids'].shape[0] == MAX_STEPS
    assert len(set(ref['lengths'].reshape(-1).tolist())) > 1
    assert not np.array_equal(ref['step_ids'], ref3['step_ids'])
    dec = cdec.Decoder(spec, p, DEV)
    smp = BeamSampling(TEMP, 2)
    eager = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=True, use_graph=False, sampling=smp)
    _check_decode(eager, ref)
    assert (eager['parent_ids'] == np.arange(N_DEC)).all()
    dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, sampling=smp)               # captures
    replay = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=True, sampling=smp)
    ctxs = dec._self_ensemble._ctxs
    assert len(ctxs) == 1 and next(iter(ctxs.values())).graph is not None
    graph = next(iter(ctxs.values())).graph
    for k in ('step_ids', 'parent_ids', 'predicted_ids', 'lengths', 'scores', 'log_probs', 'attn_hist'):
        np.testing.assert_array_equal(replay[k], eager[k], err_msg='replay: ' + k)
    other = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=False, sampling=BeamSampling(TEMP, 3))
    assert len(ctxs) == 1 and next(iter(ctxs.values())).graph is graph, 'a new seed must not build or capture anything'
    _check_decode(other, ref3)
    # Decoder.score of the sampled captions reproduces their log-probabilities (the project's 1e-3 relative fp32 bar)
    T, B = eager['predicted_ids'].shape[:2]
    caps = np.full((B * N_DEC, T + 1), -1, np.int64)
    caps[:, 0] = spec.start_id
    ids = eager['predicted_ids'].transpose(1, 2, 0).reshape(B * N_DEC, T)
    ln = eager['lengths'].reshape(-1)
    for r in range(B * N_DEC):
        caps[r, 1:1 + ln[r]] = ids[r, :ln[r]]
    rep = lambda a: dev(np.repeat(a, N_DEC, axis=0))
    sc = dec.score(rep(fm), rep(im), caps, use_graph=False)
    assert_close(sc['log_prob'].cpu().numpy().reshape(B, N_DEC), eager['log_probs'], F32_RTOL, 'Decoder.score of the samples')


def test_early_exit_keeps_the_poison():
    """Checked on the CPU: with the strong EOS bias and noise seed 6 the reference ends after 5 of 14 steps, margin 108.
    Rows past steps_executed are never written, eager, captured or replayed."""
    fm, im = _features()
    spec, cfg, p, ref = _single(56, 5.0, 6)
    T = ref['step_ids'].shape[0]
    print('reference: %d steps, rank-gap margin %.2f' % (T, ref['margin']))
    assert ref['margin'] > 1.0 and T < MAX_STEPS
    dec = cdec.Decoder(spec, p, DEV)
    for _ in range(3):
        res = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=False, sampling=BeamSampling(TEMP, 6))
        _check_decode(res, ref)
        ctx = next(iter(dec._self_ensemble._ctxs.values()))
        assert bool((ctx.step_ids[T:] == POISON).all()) and bool((ctx.parent_ids[T:] == POISON).all())
    assert ctx.graph is not None


def test_ensemble_of_two_members():
    """Two members with different head counts, weights [0.6, 0.4], noise seed 3.  Checked on the CPU: 14 steps, margin 90.9."""
    fm, im = _features()
    members = []
    for seed, geo in ((42, dict()), (43, dict(H=4))):
        spec, cfg = _spec_and_cfg(**geo)
        members.append((spec, cfg, _rand_params(cfg, seed, 3.0)))
    wts = [0.6, 0.4]
    ref = sref.sampled_reference([(p, cfg) for _, cfg, p in members], np.asarray(wts, np.float32), fm, im, N_DEC, MAX_STEPS,
                                 3, TEMP)
    print('reference rank-gap margin %.2f' % ref['margin'])
    assert ref['margin'] > 1.0 and ref['step_ids'].shape[0] == MAX_STEPS
    ens = cdec.EnsembleDecoder([cdec.Decoder(spec, p, DEV) for spec, _, p in members], wts)
    _check_decode(ens.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, sampling=BeamSampling(TEMP, 3)), ref)


def test_sampling_with_constraints():
    """min_length 6 and no repeated bigram, noise seed 5.  Checked on the CPU: 14 steps, margin 96.0; the ids differ from
    the unconstrained samples."""
    kw = dict(min_length=6, no_repeat_ngram=2)
    fm, im = _features()
    spec, cfg, p, ref = _single(75, 3.0, 5, **kw)
    print('reference rank-gap margin %.2f' % ref['margin'])
    assert ref['margin'] > 1.0 and ref['step_ids'].shape[0] == MAX_STEPS
    assert not np.array_equal(_single(75, 3.0, 5)[3]['step_ids'], ref['step_ids'])
    dec = cdec.Decoder(spec, p, DEV)
    res = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=False, constraints=BeamConstraints(**kw),
                          sampling=BeamSampling(TEMP, 5))
    _check_decode(res, ref)
    assert res['lengths'].min() >= 6


def test_the_same_captions_whatever_the_batching():
    """Images 0-3 in one batch, and as two batches of two with image_base 0 and 2: both are the reference of the four
    (noise seed 2; checked on the CPU: 14 steps, margin 164.4)."""
    a, b = _features(21), _features(22)
    fm, im = np.concatenate([a[0], b[0][:1]]), np.concatenate([a[1], b[1][:1]])
    spec, cfg = _spec_and_cfg()
    p = _rand_params(cfg, 61, 3.0)
    ref = sref.sampled_reference([(p, cfg)], np.ones(1, np.float32), fm, im, N_DEC, MAX_STEPS, 2, TEMP)
    print('reference rank-gap margin %.2f' % ref['margin'])
    assert ref['margin'] > 1.0 and ref['step_ids'].shape[0] == MAX_STEPS
    dec = cdec.Decoder(spec, p, DEV)
    smp = BeamSampling(TEMP, 2)
    whole = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=False, sampling=smp)
    _check_decode(whole, ref)
    for base in (0, 2):
        half = dec.beam_search(dev(fm[base:base + 2]), dev(im[base:base + 2]), N_DEC, MAX_STEPS, want_attention=False,
                               sampling=smp, image_base=base)
        T = half['step_ids'].shape[0]
        # (a half ends when ITS chains have ended; a finished chain emits <EOS> from then on)
        np.testing.assert_array_equal(half['predicted_ids'], whole['predicted_ids'][:T, base:base + 2])
        assert (whole['predicted_ids'][T:, base:base + 2] == spec.end_id).all()
        np.testing.assert_array_equal(half['lengths'], ref['lengths'][base:base + 2])
        assert_close(half['log_probs'], ref['log_probs'][base:base + 2], F32_RTOL, 'log_probs of a half')


def test_refused_on_the_host_and_by_the_executor():
    spec, cfg = _spec_and_cfg()
    dec = cdec.Decoder(spec, _rand_params(cfg, 61, 3.0), DEV)
    fm, im = _features()
    for kw, what in ((dict(sampling=BeamSampling(0.0, 1)), 'temperature'),
                     (dict(sampling=BeamSampling(TEMP, 1), groups=BeamGroups(2, 0.5)), 'beam groups'),
                     (dict(sampling=BeamSampling(TEMP, 1), length_penalty_weight=0.7), 'length penalty')):
        with pytest.raises(ValueError, match=what):
            dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, **kw)
    assert '_self_ensemble' not in dec.__dict__                               # refused before anything was built
    # the executor's own refusals: a length penalty in the descriptor, a null sampling
    lib = L.load()
    ens = cdec.EnsembleDecoder([dec])
    ctx = ens._ctx(fm.shape[0], N_DEC, MAX_STEPS, [(dev(fm), dev(im))], cdec.BeamOptions(sampling=BeamSampling(TEMP, 1)))

    def call(smp):
        return lib.comic_decoder_beam_sampled(ctx.descs, ctx.ptabs, ctx.fm_ptrs, ctx.im_ptrs, ctx.wts, 1, fm.shape[0], N_DEC,
                                              MAX_STEPS, None, smp, ctx.step_ids.data_ptr(), ctx.parent_ids.data_ptr(),
                                              ctx.scores.data_ptr(), ctx.lengths.data_ptr(), ctx.finished.data_ptr(),
                                              ctx.hist_ptrs, ctx.steps.data_ptr(), ctx.ws.data_ptr(), ctx.nbytes, stream())
    assert call(None) != 0 and 'null sampling' in lib.comic_last_error().decode()
    ctx.descs[0].length_penalty_weight = 0.7
    assert call(C.byref(ctx.smp)) != 0 and 'length penalty' in lib.comic_last_error().decode()
    sync()


# ------------------------------------------------------------------ model and CLI ----------------------------------------
def test_infer_cli_flags_write_both_files_in_a_directory_of_their_own(tiny_run):  # noqa: F811
    ds, run_dir, ckpt = tiny_run
    num = os.path.basename(ckpt)[len('model_compact-'):-len('.npz')]
    common = ['--infer_checkpoints_dir', run_dir, '--dataset_dir', ds, '--infer_set', 'test', '--batch_size_infer', '2',
              '--get_metric_score', '', '--infer_checkpoints', num, '--infer_beam_size', '4', '--infer_sample',
              '--infer_temperature', '0.7']
    plain_dir = os.path.join(run_dir, 'infer_test_beam_4_lpen_0.0')

    def run(seed):
        out_dir = plain_dir + '_smp_t0.7_s%d' % seed
        for name in ('captions___%s.json' % num, 'caption_samples___%s.json' % num):      # (a second run decodes again)
            if os.path.exists(os.path.join(out_dir, name)):
                os.remove(os.path.join(out_dir, name))
        _run(os.path.join(ROOT, 'src', 'infer.py'), common + ['--infer_sample_seed', str(seed)])
        return (json.load(open(os.path.join(out_dir, 'captions___%s.json' % num))),
                json.load(open(os.path.join(out_dir, 'caption_samples___%s.json' % num))))
    caps, samples = run(3)
    assert not os.path.exists(plain_dir)
    assert len(caps) == 4 and len(samples) == 4
    for cap, s in zip(caps, samples):
        assert s['image_id'] == cap['image_id'] and len(s['captions']) == 4
        assert [x['sample'] for x in s['captions']] == [0, 1, 2, 3]
        lps = [x['log_prob'] for x in s['captions']]
        assert all(np.isfinite(v) and v <= 0.0 for v in lps)
        assert s['captions'][int(np.argmax(lps))]['caption'] == cap['caption']      # the likeliest sample is THE caption
    assert run(3) == (caps, samples)                                               # the same seed: the same files
    assert run(4)[1] != samples                                                    # another seed: other samples
    with pytest.raises(ValueError, match='beam groups'):
        _run(os.path.join(ROOT, 'src', 'infer.py'), common + ['--infer_beam_groups', '2'])
    with pytest.raises(ValueError, match='length penalty'):
        _run(os.path.join(ROOT, 'src', 'infer.py'), common + ['--infer_length_penalty_weight', '0.5'])
