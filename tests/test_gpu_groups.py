"""Diverse beam search on the GPU: the grouped step (comic_beam_step_diverse) against the float64 reference of
tests/beam_groups_ref.py, its degenerate cases against the plain ensemble step, the whole decoder (Decoder / EnsembleDecoder
.beam_search(groups=)) against the reference loop, the model level and `infer.py`'s flags on the tiny dataset.

Ids are compared exactly under the rule of tests/test_gpu_ensemble.py, applied per group: every case asserts that its float64
reference separates the ranks 1 ... Wg + 1 of the PENALISED ranking by more than the bar (margin > 1) in EVERY entry and
EVERY group; no entry is excused.  The margins quoted below were computed on the CPU with this reference."""
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
from comic_amd.decoder import BeamConstraints, BeamGroups
from tests import beam_constraints_ref as bref
from tests import beam_groups_ref as gref
from tests.gpu_util import DEV, F32_RTOL, assert_close, dev, stream, sync
from tests.test_gpu_constraints import tiny_run  # noqa: F401  (the fixture: a one-epoch run on the tiny dataset)
from tests.test_gpu_ensemble import POISON, _features, _rand_params, _run, _spec_and_cfg, ref_select, run_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = 0.5
MAX_STEPS = 14

# ((n, B, W, V), G, seed): smallest; radix vocabulary with three groups and three members; the split form with two groups
# and with groups of one slot; G == W in one workgroup; three groups of three in the split form; Wg * kper = 9 * 5 = 45 > 40:
# the rescanning chunk form; more than 32 rows.  Minimum margin over init / mid and lpw 0 / 0.7, computed on the CPU:
# 47, 9.3, 9.7, 3.7, 15, 7.0, 11, 22.
CASES = [((1, 2, 4, 17), 2, 0), ((3, 3, 6, 258), 3, 0), ((2, 2, 6, 9001), 2, 0), ((2, 2, 6, 9001), 6, 0),
         ((1, 3, 4, 258), 4, 0), ((1, 2, 9, 9001), 3, 0), ((2, 2, 18, 9001), 2, 1), ((1, 33, 2, 258), 2, 0)]
STEP_CASES = [(shape, G, seed, state, lpw) for shape, G, seed in CASES for state in ('init', 'mid') for lpw in (0.0, 0.7)]


# ------------------------------------------------------------------ the grouped step ---------------------------------
def run_step_diverse(logits, wts, log_probs, finished, lengths, end_id, lpw, G, lam, bits=None, workspace=True):
    lib = L.load()
    n, B, W, V = logits.shape
    d_lg, d_lp, d_fin, d_len = dev(logits), dev(log_probs), dev(finished), dev(lengths)
    d_bits = dev(np.ascontiguousarray(bits).view(np.int32)) if bits is not None else None
    word = torch.full((B, W), -1, dtype=torch.int32, device=DEV)
    parent = torch.full((B, W), -1, dtype=torch.int32, device=DEV)
    scores = torch.zeros((B, W), dtype=torch.float32, device=DEV)
    nbytes = int(lib.comic_beam_step_ensemble_workspace(n, B, W, V))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ws_ptr, ws_bytes = (ws.data_ptr(), nbytes) if workspace else (None, 0)
    wt = (C.c_float * n)(*[float(w) for w in wts])
    grp = BeamGroups(G, lam).c_struct()
    L.check(lib.comic_beam_step_diverse(d_lg.data_ptr(), wt, n, d_lp.data_ptr(), d_fin.data_ptr(), d_len.data_ptr(),
                                        word.data_ptr(), parent.data_ptr(), scores.data_ptr(), B, W, V, end_id, float(lpw),
                                        L.ptr(d_bits), (V + 31) // 32, C.byref(grp), ws_ptr, ws_bytes, stream()),
            'beam_step_diverse')
    sync()
    return dict(word=word.cpu().numpy(), parent=parent.cpu().numpy(), scores=scores.cpu().numpy(),
                log_probs=d_lp.cpu().numpy(), finished=d_fin.cpu().numpy(), lengths=d_len.cpu().numpy(),
                split=int(lib.comic_beam_step_ensemble_path()))


def _state(c):
    return c['logits'], c['wts'], c['log_probs'], c['finished'], c['lengths'], c['end_id']


def _check_step(got, ref):
    for k in ('word', 'parent', 'finished', 'lengths'):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert_close(got['scores'], ref['scores'], F32_RTOL, 'scores')
    assert_close(got['log_probs'], ref['log_probs'], F32_RTOL, 'new log_probs')


@pytest.mark.parametrize('shape,G,seed,state,lpw', STEP_CASES)
def test_diverse_step_matches_float64(shape, G, seed, state, lpw):
    c = gref.groups_case(shape, G, state, lpw, LAM, seed)
    ref = c['ref']
    print('reference rank-gap margin %.2f (must exceed 1)' % ref['margin'])
    assert ref['margin'] > 1.0, 'the seed of this case does not separate the ranks of the float64 reference'
    if state == 'init':          # the penalty decides: a kernel that ignored it would fail the comparison below
        assert not (np.array_equal(ref['word'], c['ref0']['word']) and np.array_equal(ref['parent'], c['ref0']['parent'])), \
            'the penalty does not change what the step selects'
    got = run_step_diverse(*_state(c), lpw, G, LAM)
    # the split form runs exactly where the rule of the plain step says, on the entry-wide W * V
    assert got['split'] == (1 if (shape[3] == 9001 and lpw == 0.0) else 0)
    _check_step(got, ref)
    Wg = shape[2] // G
    assert (got['parent'] // Wg == np.arange(shape[2]) // Wg).all(), 'a parent outside the slot\'s group'


# ------------------------------------------------------------------ degenerate cases ---------------------------------
@pytest.mark.parametrize('shape', [(3, 3, 6, 258), (2, 2, 6, 9001)])
@pytest.mark.parametrize('workspace', [True, False])
def test_one_group_is_the_ensemble_step_to_the_bit(shape, workspace):
    for state in ('init', 'mid'):
        c = gref.groups_inputs(shape, 1, state)
        plain = run_step(*_state(c), 0.0, workspace=workspace)
        one = run_step_diverse(*_state(c), 0.0, 1, LAM, workspace=workspace)
        assert plain['split'] == (1 if shape[3] == 9001 and workspace else 0)
        for k in ('word', 'parent', 'finished', 'lengths', 'scores', 'log_probs', 'split'):
            np.testing.assert_array_equal(one[k], plain[k], err_msg=k)


@functools.lru_cache(maxsize=None)
def twin_case(shape):
    """Two groups with the SAME logits rows and state (group 1 a copy of group 0), mid-decode."""
    c = dict(gref.groups_inputs(shape, 2, 'mid'))
    Wg = shape[2] // 2
    for k in ('logits', 'log_probs', 'finished', 'lengths'):
        a = c[k].copy()
        if k == 'logits':
            a[:, :, Wg:] = a[:, :, :Wg]
        else:
            a[:, Wg:] = a[:, :Wg]
        c[k] = a
    c['ref'] = gref.ref_select_groups(gref.ref_step_lp(c['logits'], c['wts']), c['log_probs'], c['finished'], c['lengths'],
                                      c['end_id'], 0.0, 2, 0.0)
    return c


@pytest.mark.parametrize('shape', [(3, 3, 6, 258), (2, 2, 6, 9001)])
def test_zero_diversity_makes_the_groups_equal(shape):
    """Checked on the CPU: margins 22.5 and 118.6."""
    c = twin_case(shape)
    print('reference rank-gap margin %.2f (must exceed 1)' % c['ref']['margin'])
    assert c['ref']['margin'] > 1.0
    got = run_step_diverse(*_state(c), 0.0, 2, 0.0)
    _check_step(got, c['ref'])
    Wg = shape[2] // 2
    np.testing.assert_array_equal(got['parent'][:, Wg:], got['parent'][:, :Wg] + Wg)
    for k in ('word', 'finished', 'lengths', 'scores', 'log_probs'):
        np.testing.assert_array_equal(got[k][:, Wg:], got[k][:, :Wg], err_msg=k)


@pytest.mark.parametrize('shape,G,seed', [((3, 3, 6, 258), 3, 0), ((2, 2, 6, 9001), 2, 0), ((2, 2, 18, 9001), 2, 1)])
def test_group_0_is_the_ensemble_step_of_its_width(shape, G, seed):
    """No penalty ever reaches group 0: its rows are comic_beam_step_ensemble at width Wg on the same logits rows."""
    Wg = shape[2] // G
    for state in ('init', 'mid'):
        c = gref.groups_case(shape, G, state, 0.0, LAM, seed)
        assert c['ref']['margin'] > 1.0
        got = run_step_diverse(*_state(c), 0.0, G, LAM)
        narrow = run_step(np.ascontiguousarray(c['logits'][:, :, :Wg]), c['wts'], c['log_probs'][:, :Wg].copy(),
                          c['finished'][:, :Wg].copy(), c['lengths'][:, :Wg].copy(), c['end_id'], 0.0)
        for k in ('word', 'parent', 'finished', 'lengths'):
            np.testing.assert_array_equal(got[k][:, :Wg], narrow[k], err_msg=k)
        assert_close(got['scores'][:, :Wg], narrow['scores'], F32_RTOL, 'scores')
        assert_close(got['log_probs'][:, :Wg], narrow['log_probs'], F32_RTOL, 'new log_probs')


# ------------------------------------------------------------------ with bans ------------------------------------------
@functools.lru_cache(maxsize=None)
def banned_case(shape, G, state):
    """Half of all candidates banned, and with them every candidate the unbanned grouped reference selects."""
    c = gref.groups_case(shape, G, state, 0.0, LAM)
    n, B, W, V = shape
    mask = np.random.default_rng(1).random((B, W, V)) < 0.5
    mask[np.arange(B)[:, None], c['ref']['parent'], c['ref']['word']] = True
    live = c['finished'] == 0
    lp = np.where(mask & live[:, :, None], -np.inf, c['lp'])
    return c, mask, gref.ref_select_groups(lp, c['log_probs'], c['finished'], c['lengths'], c['end_id'], 0.0, G, LAM)


@pytest.mark.parametrize('shape,G,state', [((3, 3, 6, 258), 3, 'mid'), ((2, 2, 6, 9001), 2, 'init')])
def test_diverse_step_under_a_ban_mask(shape, G, state):
    """Checked on the CPU: margins 3.1 and 12.8."""
    c, mask, ref = banned_case(shape, G, state)
    print('reference rank-gap margin %.2f (must exceed 1)' % ref['margin'])
    assert ref['margin'] > 1.0
    assert not np.array_equal(ref['word'], c['ref']['word']), 'the mask does not change what the step selects'
    n, B, W, V = shape
    got = run_step_diverse(*_state(c), 0.0, G, LAM, bits=bref.pack_bits(mask.reshape(B * W, V)))
    assert got['split'] == (1 if V == 9001 else 0)
    _check_step(got, ref)
    bidx = np.arange(B)[:, None]
    live_parent = c['finished'][bidx, got['parent']] == 0
    assert live_parent.any()
    assert not (mask[bidx, got['parent'], got['word']] & live_parent).any(), 'a banned candidate of a live beam was selected'


@pytest.mark.parametrize('shape,G', [((3, 3, 6, 258), 3), ((2, 2, 6, 9001), 2)])
def test_all_zero_mask_is_no_mask_to_the_bit(shape, G):
    n, B, W, V = shape
    for state in ('init', 'mid'):
        c = gref.groups_inputs(shape, G, state)
        none = run_step_diverse(*_state(c), 0.0, G, LAM)
        zero = run_step_diverse(*_state(c), 0.0, G, LAM, bits=np.zeros((B * W, (V + 31) // 32), np.uint32))
        for k in ('word', 'parent', 'finished', 'lengths', 'scores', 'log_probs', 'split'):
            np.testing.assert_array_equal(zero[k], none[k], err_msg=k)


# ------------------------------------------------------------------ refusals -------------------------------------------
def test_step_refuses_bad_groups():
    lib = L.load()
    B, W, V = 1, 6, 17
    buf = torch.zeros(4096, dtype=torch.int32, device=DEV)
    wt = (C.c_float * 1)(1.0)

    def call(grp, W=W, V=V):
        p = buf.data_ptr()
        return lib.comic_beam_step_diverse(p, wt, 1, p, p, p, p, p, p, B, W, V, V - 1, 0.0, None, 0,
                                           C.byref(grp) if grp is not None else None, None, 0, stream())
    for grp, kw, what in ((None, {}, 'null groups'),
                          (L.BeamGroups(0, 0.5), {}, 'groups must be at least 1'),
                          (L.BeamGroups(12, 0.5), {}, 'groups 12 exceeds'),
                          (L.BeamGroups(4, 0.5), {}, 'groups 4 does not divide'),
                          (L.BeamGroups(2, -0.5), {}, 'diversity'),
                          (L.BeamGroups(2, float('nan')), {}, 'diversity'),
                          (L.BeamGroups(2, float('inf')), {}, 'diversity'),
                          (L.BeamGroups(2, 0.5), dict(W=64, V=17), 'group\'s width')):
        assert call(grp, **kw) != 0
        assert what in lib.comic_last_error().decode(), (what, lib.comic_last_error())
    sync()


# ------------------------------------------------------------------ the whole decoder ------------------------------------
W_DEC, G_DEC = 6, 3


def _check_decode(res, ref):
    assert res['step_ids'].shape[0] == ref['step_ids'].shape[0]                # steps_executed
    np.testing.assert_array_equal(res['step_ids'], ref['step_ids'])
    np.testing.assert_array_equal(res['parent_ids'], ref['parent_ids'])
    np.testing.assert_array_equal(res['lengths'], ref['lengths'])
    fin = np.isfinite(ref['scores'])
    assert_close(np.where(fin, res['scores'], 0), np.where(fin, ref['scores'], 0), F32_RTOL, 'scores')
    assert res['groups'] == G_DEC
    assert_close(res['log_probs'], ref['log_probs'], F32_RTOL, 'final log_probs')


def _differs(a, b):
    return a['step_ids'].shape != b['step_ids'].shape or not np.array_equal(a['step_ids'], b['step_ids'])


def _single(seed, eos_bias, **cons):
    fm, im = _features()
    spec, cfg = _spec_and_cfg()
    p = _rand_params(cfg, seed, eos_bias)
    ref = gref.diverse_reference([(p, cfg)], np.ones(1, np.float32), fm, im, W_DEC, MAX_STEPS, G_DEC, LAM, **cons)
    return spec, cfg, p, ref


def test_single_decoder_three_groups():
    """Checked on the CPU: 14 steps, finished and live beams side by side, margin 27.7; the ids differ from diversity 0.
    The third call replays the captured graph."""
    fm, im = _features()
    spec, cfg, p, ref = _single(61, 3.0)
    print('reference rank-gap margin over %d steps: %.2f (must exceed 1)' % (ref['step_ids'].shape[0], ref['margin']))
    assert ref['margin'] > 1.0 and ref['step_ids'].shape[0] == MAX_STEPS
    assert len(set(ref['lengths'].reshape(-1).tolist())) > 1
    assert _differs(gref.diverse_reference([(p, cfg)], np.ones(1, np.float32), fm, im, W_DEC, MAX_STEPS, G_DEC, 0.0), ref)
    dec = cdec.Decoder(spec, p, DEV)
    grp = BeamGroups(G_DEC, LAM)
    eager = dec.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, want_attention=True, use_graph=False, groups=grp)
    _check_decode(eager, ref)
    Wg = W_DEC // G_DEC
    assert (eager['parent_ids'] // Wg == np.arange(W_DEC) // Wg).all()
    dec.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, groups=grp)             # captures
    replay = dec.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, want_attention=True, groups=grp)
    again = dec.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, want_attention=True, groups=grp)
    ctxs = dec._self_ensemble._ctxs
    assert len(ctxs) == 1 and next(iter(ctxs.values())).graph is not None
    for k in ('step_ids', 'parent_ids', 'predicted_ids', 'lengths', 'scores', 'log_probs', 'attn_hist'):
        np.testing.assert_array_equal(replay[k], eager[k], err_msg='replay: ' + k)
        np.testing.assert_array_equal(again[k], replay[k], err_msg='second replay: ' + k)


def test_early_exit_keeps_the_poison():
    """Checked on the CPU: with the strong EOS bias the reference ends after 2 of 14 steps, margin 122.  Rows past
    steps_executed are never written, eager, captured or replayed."""
    fm, im = _features()
    spec, cfg, p, ref = _single(56, 5.0)
    T = ref['step_ids'].shape[0]
    print('reference: %d steps, rank-gap margin %.2f' % (T, ref['margin']))
    assert ref['margin'] > 1.0 and T < MAX_STEPS
    dec = cdec.Decoder(spec, p, DEV)
    for _ in range(3):
        res = dec.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, want_attention=False, groups=BeamGroups(G_DEC, LAM))
        _check_decode(res, ref)
        ctx = next(iter(dec._self_ensemble._ctxs.values()))
        assert bool((ctx.step_ids[T:] == POISON).all()) and bool((ctx.parent_ids[T:] == POISON).all())
    assert ctx.graph is not None


def test_ensemble_of_two_members():
    """Two members with different head counts, weights [0.6, 0.4].  Checked on the CPU: 14 steps, margin 3.10."""
    fm, im = _features()
    members = []
    for seed, geo in ((42, dict()), (43, dict(H=4))):
        spec, cfg = _spec_and_cfg(**geo)
        members.append((spec, cfg, _rand_params(cfg, seed, 3.0)))
    wts = [0.6, 0.4]
    ref = gref.diverse_reference([(p, cfg) for _, cfg, p in members], np.asarray(wts, np.float32), fm, im, W_DEC, MAX_STEPS,
                                 G_DEC, LAM)
    print('reference rank-gap margin %.2f' % ref['margin'])
    assert ref['margin'] > 1.0 and ref['step_ids'].shape[0] == MAX_STEPS
    ens = cdec.EnsembleDecoder([cdec.Decoder(spec, p, DEV) for spec, _, p in members], wts)
    _check_decode(ens.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, groups=BeamGroups(G_DEC, LAM)), ref)


def test_groups_with_constraints_and_group_0_alone():
    """BeamGroups(3, 0.5) with min_length 6 and no repeated bigram.  Checked on the CPU: 14 steps, margin 3.18; the ids
    differ from the unconstrained grouped decode and from diversity 0.  Group 0 of the run is beam search of width 2
    under the same constraints through the same executor."""
    kw = dict(min_length=6, no_repeat_ngram=2)
    fm, im = _features()
    spec, cfg, p, ref = _single(75, 3.0, **kw)
    print('reference rank-gap margin %.2f' % ref['margin'])
    assert ref['margin'] > 1.0 and ref['step_ids'].shape[0] == MAX_STEPS
    one = np.ones(1, np.float32)
    assert _differs(gref.diverse_reference([(p, cfg)], one, fm, im, W_DEC, MAX_STEPS, G_DEC, LAM), ref)
    assert _differs(gref.diverse_reference([(p, cfg)], one, fm, im, W_DEC, MAX_STEPS, G_DEC, 0.0, **kw), ref)
    dec = cdec.Decoder(spec, p, DEV)
    cons = BeamConstraints(**kw)
    res = dec.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, want_attention=False, constraints=cons,
                          groups=BeamGroups(G_DEC, LAM))
    _check_decode(res, ref)
    Wg = W_DEC // G_DEC
    narrow = dec.beam_search(dev(fm), dev(im), Wg, MAX_STEPS, want_attention=False, constraints=cons)
    assert narrow['groups'] == 1 and narrow['step_ids'].shape[0] <= res['step_ids'].shape[0]
    T = narrow['step_ids'].shape[0]
    for k in ('step_ids', 'parent_ids'):
        np.testing.assert_array_equal(res[k][:T, :, :Wg], narrow[k], err_msg=k)
    np.testing.assert_array_equal(res['lengths'][:, :Wg], narrow['lengths'])
    assert_close(res['scores'][:T, :, :Wg], narrow['scores'], F32_RTOL, 'scores of group 0')


def test_refused_on_the_host():
    spec, cfg = _spec_and_cfg()
    dec = cdec.Decoder(spec, _rand_params(cfg, 61, 3.0), DEV)
    fm, im = _features()
    for grp, what in ((BeamGroups(4, 0.5), 'groups 4 does not divide'), (BeamGroups(2, -1.0), 'diversity'),
                      (BeamGroups(0, 0.5), 'groups must be')):
        with pytest.raises(ValueError, match=what):
            dec.beam_search(dev(fm), dev(im), W_DEC, MAX_STEPS, groups=grp)
    assert '_self_ensemble' not in dec.__dict__                               # refused before anything was built


def test_none_and_one_group_change_nothing():
    spec, cfg = _spec_and_cfg()
    p = _rand_params(cfg, 5, 3.0)
    fm, im = _features()
    dec = cdec.Decoder(spec, p, DEV)
    ens = cdec.EnsembleDecoder([dec, dec])
    for run, kw in ((dec.beam_search, dict(want_attention=False)), (ens.beam_search, dict())):
        base = run(dev(fm), dev(im), W_DEC, MAX_STEPS, use_graph=False, **kw)
        assert base['groups'] == 1 and 'log_probs' not in base
        for grp in (None, BeamGroups(), BeamGroups(1, 0.5)):
            res = run(dev(fm), dev(im), W_DEC, MAX_STEPS, use_graph=False, groups=grp, **kw)
            assert sorted(res) == sorted(base)
            for k in base:
                np.testing.assert_array_equal(res[k], base[k], err_msg=k)
    plain_key = cdec.BeamOptions().ctx_key()                                      # the plain contexts only
    assert '_self_ensemble' not in dec.__dict__ and all(k[3] == plain_key for k in ens._ctxs)


# ------------------------------------------------------------------ model and CLI ----------------------------------------
def test_infer_cli_flags_write_both_files_in_a_directory_of_their_own(tiny_run):  # noqa: F811
    ds, run_dir, ckpt = tiny_run
    num = os.path.basename(ckpt)[len('model_compact-'):-len('.npz')]
    common = ['--infer_checkpoints_dir', run_dir, '--dataset_dir', ds, '--infer_set', 'test', '--batch_size_infer', '2',
              '--get_metric_score', '', '--infer_checkpoints', num, '--infer_beam_size', '6']
    _run(os.path.join(ROOT, 'src', 'infer.py'), common + ['--infer_beam_groups', '3', '--infer_diversity', '0.5'])
    plain_dir = os.path.join(run_dir, 'infer_test_beam_6_lpen_0.0')
    grp_dir = plain_dir + '_grp3_div0.5'
    assert not os.path.exists(plain_dir)
    caps = json.load(open(os.path.join(grp_dir, 'captions___%s.json' % num)))
    groups = json.load(open(os.path.join(grp_dir, 'caption_groups___%s.json' % num)))
    assert len(caps) == 4 and len(groups) == 4
    for cap, g in zip(caps, groups):
        assert g['image_id'] == cap['image_id'] and len(g['captions']) == 3
        assert [x['group'] for x in g['captions']] == [0, 1, 2]
        assert g['captions'][0]['caption'] == cap['caption']                   # group 0's best is THE caption
        for x in g['captions']:
            assert np.isfinite(x['score']) and np.isfinite(x['log_prob']) and x['log_prob'] <= 0.0
            assert x['score'] <= x['log_prob'] + 1e-6                          # a rank is a total minus a penalty >= 0
