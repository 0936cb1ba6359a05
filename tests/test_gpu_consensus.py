"""Consensus (minimum-Bayes-risk) selection on the GPU: the operator (comic_caption_consensus through Decoder.consensus)
against the float64 reference of tests/consensus_ref.py, the decoders (Decoder / EnsembleDecoder.beam_search(consensus=)),
CaptionModel._decode_features and `infer.py`'s flags on the tiny dataset.

Bounds.  `utility` within 1e-10 absolute of the reference: at most 4 * 64 products per pair and 31 pairs per sum, a few ulp
each on values <= 10, plus the difference between the device's and the host's exp, give about 1e-11; 1e-10 leaves one order.
`best` must be a slot whose REFERENCE utility is within 1e-10 of the reference maximum, and must equal the reference argmax
wherever the reference's two largest utilities differ by more than 1e-6; test_the_reference_separates_most_images asserts,
on the reference alone, that at least three quarters of ALL the images the operator test runs are such."""
import functools
import glob
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import comic_amd._lib as L
from comic_amd import decoder as cdec
from comic_amd.decoder import BeamSampling, Consensus, NgramIdf
from tests import consensus_ref as cr
from tests.gpu_util import DEV, dev, stream, sync
from tests.test_gpu_constraints import tiny_run  # noqa: F401  (the fixture: a one-epoch run on the tiny dataset)
from tests.test_gpu_ensemble import _features, _rand_params, _run, _spec_and_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, GAP = 1e-10, 1e-6
END = 0
REF_LEN = 40

# (V, T, W, stride, B): the four shapes of the issue at B = 5; W = 1, W = 2 (a small alphabet: repeats break the symmetry),
# T = 1; B = 1; U at the bound of 64 units, once
# with the most candidates (137 KB of LDS) and once at stride 2
SHAPES = [(12, 12, 8, 1, 5), (8, 16, 6, 2, 5), (6, 18, 7, 3, 5), (30, 20, 32, 1, 5),
          (12, 12, 1, 1, 5), (4, 16, 2, 1, 5), (12, 1, 4, 1, 5), (12, 12, 8, 1, 1),
          (5, 64, 32, 1, 1), (6, 128, 4, 2, 2)]
MODES = ['uniform', 'uniform_idf', 'posterior', 'posterior_idf']


def case_ids(V, T, W, stride, B, seed=0):
    """Random ids from a small alphabet -- at a stride above 1 random WORDS from a list of V words of `stride` such
    tokens, so that whole units do recur -- random first-<EOS> positions in [0, T] (a partial last word included);
    candidate 0 of image 0 is empty and candidate 1 runs to T; the last candidate of image 0 repeats one unit (tf > 1)
    and the one before it holds that unit once; images with b % 4 == 1 hold one duplicated candidate."""
    rng = np.random.default_rng(1000 * V + 10 * T + W + seed)
    if stride == 1:
        ids = rng.integers(1, V, (T, B, W)).astype(np.int32)
    else:
        words = rng.integers(1, V, (V, stride))
        n = -(-T // stride)
        ids = words[rng.integers(0, V, (n, B, W))].transpose(0, 3, 1, 2).reshape(n * stride, B, W)[:T].astype(np.int32)
    ends = rng.integers(0, T + 1, (B, W))
    if W >= 2:
        ends[0, 0], ends[0, 1] = 0, T
    if W >= 4:
        ends[0, W - 1] = ends[0, W - 2] = T
        ids[:, 0, W - 1] = 1
        ids[T // 2:, 0, W - 1] = ids[T // 2:, 0, W - 3]
        ids[:stride, 0, W - 2] = 1
    for b in range(B):
        for w in range(W):
            ids[ends[b, w]:, b, w] = END
        if b % 4 == 1 and W >= 2:
            ids[:, b, W - 1] = ids[:, b, 0]
    return ids


def case_table(ids, stride, V, seed=0, wrap=False):
    """A table over n-grams of the case: every third distinct n-gram of its candidates (a fifth of them with df = 1, one
    with df = 0, the others with a df in [2, REF_LEN]) and as many n-grams that occur nowhere (they hold token V + 3).
    wrap: instead, the four shortest n-grams of the case whose keys share the last home slot of the minimum capacity 8."""
    rng = np.random.default_rng(7 + seed)
    T, B, W = ids.shape
    present = {}
    for b in range(B):
        for w in range(W):
            u = cr.units(ids[:, b, w], END, stride)
            for k in range(1, 5):
                for i in range(len(u) - k + 1):
                    toks = [t for unit in u[i:i + k] for t in unit]
                    present.setdefault(cr.ngram_key(toks), toks)
    keys = sorted(present)
    log_ref = math.log(float(REF_LEN))
    if wrap:
        pick = sorted((k for k in keys if k & 7 == 7), key=lambda k: (len(present[k]), k))[:4]     # the shortest: they recur
        assert len(pick) == 4
        entries = {k: log_ref - math.log(float(2 + n)) for n, k in enumerate(pick)}
        table = cr.build_table(entries)
        assert len(table[0]) == 8 and all(table[0][s] != 0 for s in (7, 0, 1, 2)), 'the probe sequence must wrap'
        return table
    entries = {}
    for n, k in enumerate(keys[::3]):
        df = 1.0 if n % 5 == 0 else float(rng.integers(2, REF_LEN + 1))
        if n == 1:
            df = 0.0
        entries[k] = log_ref - math.log(max(1.0, df))
    for n in range(len(keys[::3])):
        m = int(rng.integers(1, 5)) * stride
        entries.setdefault(cr.ngram_key([V + 3] + [int(x) for x in rng.integers(1, V, m - 1)]), 0.5)
    return cr.build_table(entries)


def case_log_probs(B, W, seed=0):
    """Final log-probabilities with one -inf slot per image (the slot moves with the image)."""
    rng = np.random.default_rng(77 + seed)
    lp = (-8.0 * rng.random((B, W))).astype(np.float32)
    if W >= 2:
        lp[np.arange(B), np.arange(B) % W] = -np.inf
    return lp


@functools.lru_cache(maxsize=None)
def case(shape, mode, wrap=False):
    """ids, table, log_probs and the reference of a case, computed once."""
    V, T, W, stride, B = shape
    ids = case_ids(V, T, W, stride, B)
    table = case_table(ids, stride, V, wrap=wrap) if mode.endswith('_idf') else None
    lp = case_log_probs(B, W) if mode.startswith('posterior') else None
    util, best = cr.consensus(ids, END, stride, lp, table, math.log(float(REF_LEN)))
    for a in (ids, util, best):
        a.setflags(write=False)
    return dict(ids=ids, table=table, lp=lp, util=util, best=best, stride=stride)


def _cons(c, mode):
    idf = None
    if c['table'] is not None:
        idf = NgramIdf(c['table'][0], c['table'][1], math.log(float(REF_LEN)), c['stride'])
    return Consensus(mode.split('_')[0], c['stride'], idf)


@functools.lru_cache(maxsize=None)
def _decoder():
    spec, cfg = _spec_and_cfg()
    return cdec.Decoder(spec, _rand_params(cfg, 61, 3.0), DEV)


class _Op:
    """Decoder.consensus under another end_id than the tiny decoder's (the operator reads spec.end_id)."""
    def __init__(self):
        d = _decoder()
        self.lib, self.torch, self.device = d.lib, d.torch, d.device
        self.spec = type('S', (), dict(end_id=END))()
    consensus = cdec.Decoder.consensus


def _separated(util):
    """Per image: the reference's two largest finite utilities differ by more than GAP (images of one candidate: True)."""
    out = []
    for row in util:
        v = np.sort(row[np.isfinite(row)])[::-1]
        out.append(len(v) < 2 or v[0] - v[1] > GAP)
    return np.array(out)


def _check(got_u, got_b, c):
    ru, rb = c['util'], c['best']
    assert got_u.dtype == np.float64 and got_b.dtype == np.int32 and got_u.shape == ru.shape and got_b.shape == rb.shape
    np.testing.assert_array_equal(np.isneginf(got_u), np.isneginf(ru))
    fin = np.isfinite(ru)
    assert np.isfinite(got_u[fin]).all()
    err = float(np.abs(got_u[fin] - ru[fin]).max()) if fin.any() else 0.0
    sep = _separated(ru)
    print('max |utility - reference| = %.3e (bound %.0e); %d of %d images separated by more than %.0e'
          % (err, TOL, int(sep.sum()), len(sep), GAP))
    assert err <= TOL
    B = ru.shape[0]
    assert ((0 <= got_b) & (got_b < ru.shape[1])).all()
    chosen = ru[np.arange(B), got_b]
    top = np.where(fin, ru, -np.inf).max(axis=1)
    ok = np.where(np.isfinite(top), chosen >= top - TOL, got_b == 0)
    assert ok.all(), 'best is not a slot of (nearly) the largest reference utility: %r against %r' % (got_b, rb)
    np.testing.assert_array_equal(got_b[sep], rb[sep])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', SHAPES)
def test_operator_matches_the_reference(shape, mode):
    c = case(shape, mode)
    op = _Op()
    cons = _cons(c, mode)
    u, b = op.consensus(dev(np.array(c['ids'])), cons, c['lp'])
    _check(u, b, c)
    # two runs give the same bits; a numpy array is taken as a device tensor is
    u2, b2 = op.consensus(np.array(c['ids']), cons, c['lp'])
    np.testing.assert_array_equal(u2.view(np.int64), u.view(np.int64))
    np.testing.assert_array_equal(b2, b)
    # the same images in another batch order give the same rows
    B = c['ids'].shape[1]
    if B > 1:
        perm = np.roll(np.arange(B), 2)
        u3, b3 = op.consensus(np.ascontiguousarray(c['ids'][:, perm]), cons, None if c['lp'] is None else c['lp'][perm])
        np.testing.assert_array_equal(u3.view(np.int64), u[perm].view(np.int64))
        np.testing.assert_array_equal(b3, b[perm])


def test_the_reference_separates_most_images():
    """On the reference alone, over EVERY image of every shape and mode the operator test runs: at least three quarters
    have a top utility that beats the runner-up by more than 1e-6, so `best` is pinned to the reference argmax there.
    The W = 1 images count as pinned (one slot); without them the share must hold as well.  The rest are ties by
    construction: T = 1 in the uniform modes (a top candidate that matches anything has a twin), the image whose top
    candidate is duplicated, two candidates whose overlap holds no repeated n-gram (the similarity is then symmetric)."""
    sep, many = [], []
    for shape in SHAPES:
        for mode in MODES:
            s = _separated(case(shape, mode)['util']).tolist()
            sep += s
            many += s if shape[2] >= 2 else []
    print('%d of %d images separated; %d of %d with two candidates or more' % (sum(sep), len(sep), sum(many), len(many)))
    assert len(sep) == 4 * sum(shape[4] for shape in SHAPES)
    assert np.mean(sep) >= 0.75 and np.mean(many) >= 0.75


@pytest.mark.parametrize('shape', [(12, 12, 8, 1, 5), (8, 16, 6, 2, 5)])
def test_probing_wraps_past_the_end_of_a_minimum_table(shape):
    """Four keys that share home slot 7 of a table of capacity 8 (twice the entries): they sit in slots 7, 0, 1, 2."""
    c = case(shape, 'uniform_idf', True)
    plain = case(shape, 'uniform')
    assert np.abs(c['util'] - plain['util']).max() > 1e-6, 'the table must change the utilities'
    u, b = _Op().consensus(dev(np.array(c['ids'])), _cons(c, 'uniform_idf'))
    _check(u, b, c)


def test_the_entry_refuses_before_any_launch():
    lib = L.load()
    buf = torch.zeros(1 << 16, dtype=torch.int32, device=DEV)
    p = buf.data_ptr()

    def call(T=12, B=2, W=4, stride=1, lp=None, mode=0, keys=None, g=None, cap=0, sigma=6.0, ids=p):
        return lib.comic_caption_consensus(ids, T, B, W, END, stride, lp, mode, keys, g, cap, 1.0, sigma, p, p, None, 0,
                                           stream())
    assert call() == 0
    for kw, what in ((dict(W=33), 'W = 33'), (dict(W=0), 'W = 0'), (dict(T=65), 'T = 65'), (dict(T=129, stride=2), 'T = 129'),
                     (dict(stride=0), 'stride'), (dict(stride=9, T=9), 'stride'), (dict(mode=2), 'weights_mode'),
                     (dict(mode=1), 'posterior'), (dict(sigma=0.0), 'sigma'), (dict(keys=p, g=p, cap=12), 'power of two'),
                     (dict(keys=p, g=None, cap=8), 'g values'), (dict(ids=None), 'NULL')):
        assert call(**kw) == 2, kw
        assert what in lib.comic_last_error().decode(), (what, lib.comic_last_error())
    assert lib.comic_caption_consensus_workspace(2, 33, 12, 1) == -1
    assert lib.comic_caption_consensus_workspace(2, 32, 65, 1) == -1
    assert lib.comic_caption_consensus_workspace(2, 32, 64, 1) == 0
    sync()


# ------------------------------------------------------------------ the decoders ---------------------------------------
N_DEC, TEMP, MAX_STEPS = 4, 0.8, 14


def _same_but_for_consensus(res, base):
    assert sorted(set(res) - {'consensus', 'consensus_best'}) == sorted(base)
    for k in base:
        np.testing.assert_array_equal(res[k], base[k], err_msg=k)


@pytest.mark.parametrize('weights', ['uniform', 'posterior'])
def test_beam_search_with_sampling_carries_the_operator_on_its_own_ids(weights):
    """consensus / consensus_best are the operator on the returned predicted_ids (and log_probs); every other key is the
    decode without consensus=, bit for bit; the reference agrees."""
    fm, im = _features()
    dec = _decoder()
    smp = BeamSampling(TEMP, 2)
    cons = Consensus(weights)
    base = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=True, use_graph=False, sampling=smp)
    res = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=True, use_graph=False, sampling=smp,
                          consensus=cons)
    _same_but_for_consensus(res, base)
    lp = res['log_probs'] if weights == 'posterior' else None
    u, b = dec.consensus(res['predicted_ids'], cons, lp)
    np.testing.assert_array_equal(res['consensus'].view(np.int64), u.view(np.int64))
    np.testing.assert_array_equal(res['consensus_best'], b)
    ru, rb = cr.consensus(res['predicted_ids'], dec.spec.end_id, 1, lp)
    _check(u, b, dict(util=ru, best=rb))
    assert len(set(map(bytes, res['predicted_ids'].transpose(1, 2, 0).reshape(-1, res['predicted_ids'].shape[0])))) > 2
    # the launch stays outside the captured graph: capture, replay, the same result
    for _ in range(2):
        again = dec.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, want_attention=True, sampling=smp, consensus=cons)
    for k in res:
        np.testing.assert_array_equal(again[k], res[k], err_msg='replay: ' + k)


def test_plain_beam_search_and_an_ensemble_of_two():
    fm, im = _features()
    dec = _decoder()
    cons = Consensus('posterior')
    base = dec.beam_search(dev(fm), dev(im), 3, MAX_STEPS, want_attention=False, use_graph=False)
    res = dec.beam_search(dev(fm), dev(im), 3, MAX_STEPS, want_attention=False, use_graph=False, consensus=cons)
    _same_but_for_consensus(res, base)
    u, b = dec.consensus(res['predicted_ids'], cons, res['scores'][-1])
    np.testing.assert_array_equal(res['consensus'].view(np.int64), u.view(np.int64))
    np.testing.assert_array_equal(res['consensus_best'], b)
    members = []
    for seed, geo in ((42, dict()), (43, dict(H=4))):
        spec, cfg = _spec_and_cfg(**geo)
        members.append(cdec.Decoder(spec, _rand_params(cfg, seed, 3.0), DEV))
    ens = cdec.EnsembleDecoder(members, [0.6, 0.4])
    smp, cons = BeamSampling(TEMP, 3), Consensus()
    base = ens.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, use_graph=False, sampling=smp)
    res = ens.beam_search(dev(fm), dev(im), N_DEC, MAX_STEPS, use_graph=False, sampling=smp, consensus=cons)
    _same_but_for_consensus(res, base)
    u, b = members[0].consensus(res['predicted_ids'], cons)
    np.testing.assert_array_equal(res['consensus'].view(np.int64), u.view(np.int64))
    np.testing.assert_array_equal(res['consensus_best'], b)
    ru, rb = cr.consensus(res['predicted_ids'], ens.spec.end_id, 1)
    _check(u, b, dict(util=ru, best=rb))


def test_refused_on_the_host_before_anything_is_built():
    spec, cfg = _spec_and_cfg()
    dec = cdec.Decoder(spec, _rand_params(cfg, 61, 3.0), DEV)
    fm, im = _features()
    for beam, steps, cons, what in ((33, MAX_STEPS, Consensus(), 'beam'), (4, 65, Consensus(), 'max_steps'),
                                    (4, MAX_STEPS, Consensus('map'), 'weights'), (4, MAX_STEPS, Consensus(stride=9), 'stride')):
        with pytest.raises(ValueError, match=what):
            dec.beam_search(dev(fm), dev(im), beam, steps, sampling=BeamSampling(TEMP, 1), consensus=cons)
    assert '_self_ensemble' not in dec.__dict__
    with pytest.raises(ValueError, match='log_probs'):
        dec.consensus(np.zeros((4, 1, 3), np.int32), Consensus('posterior'))


# ------------------------------------------------------------------ model and CLI ----------------------------------------
def _df_pickle(ds):
    found = glob.glob(os.path.join(ds, 'captions', '*scst-words*.p'))
    assert len(found) == 1, found
    return found[0]


def test_decode_features_returns_the_consensus_best_sample(tiny_run):  # noqa: F811
    import importlib.util
    from comic_amd import configuration as conf, inputs, model as mdl
    ds, run_dir, ckpt = tiny_run
    sp = importlib.util.spec_from_file_location('cli_infer_consensus', os.path.join(ROOT, 'src', 'infer.py'))
    cli = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(cli)
    df = _df_pickle(ds)
    args = cli.create_parser().parse_args(['--infer_checkpoints_dir', run_dir, '--dataset_dir', ds, '--infer_set', 'test',
                                           '--batch_size_infer', '2', '--infer_beam_size', '4', '--infer_sample',
                                           '--infer_temperature', '1.5', '--infer_consensus', '--infer_consensus_df', df])
    c = conf.load_config(os.path.join(run_dir, 'config.pkl'))
    c.__dict__.update({k: v for k, v in args.__dict__.items() if v is not None})
    mdl.reset_default_graph()
    man = inputs.InputManager(c, is_inference=True)
    try:
        c = man.config
        cons = cdec.consensus_from_config(c)
        assert cons.weights == 'uniform' and cons.idf is not None and cons.idf.kept > 0
        assert cons.stride == cdec.word_stride(c, c.wtoi) and c.token_type == 'radix'
        smp = cdec.sampling_from_config(c)
        man.enable_device_preprocess(DEV)
        c.resume_training = False
        c.checkpoint_path = ckpt
        m = mdl.CaptionModel(c, mode='infer', batch_ops=man.batch_infer, reuse=False, name='inference', device=DEV)
        m.restore_model()
        im_embed, fm = m._next_infer_features()
        ids, attn = m._decode_features(im_embed, fm, 4, c.infer_max_length, top_beam=True, want_attention=True,
                                       options=cdec.BeamOptions(sampling=smp, consensus=cons))
        out = m.sample_output
        # the same decode once more, raw (the noise is keyed by the seed and the image's index, both the same)
        raw = m.decoder.beam_search(fm, im_embed, 4, m.decoder.max_iterations(c.infer_max_length, len(c.wtoi)),
                                    want_attention=True, sampling=smp, consensus=cons)
        with pytest.raises(ValueError, match='sampl'):
            m._decode_features(im_embed, fm, 4, c.infer_max_length, options=cdec.BeamOptions(consensus=cons))
    finally:
        man.close()
        mdl.reset_default_graph()
    B = ids.shape[0]
    u, b = m.decoder.consensus(np.ascontiguousarray(out['ids'].transpose(2, 0, 1)), cons)
    np.testing.assert_array_equal(out['consensus'].view(np.int64), u.view(np.int64))
    np.testing.assert_array_equal(ids, out['ids'][np.arange(B), b])
    ru, rb = cr.consensus(out['ids'].transpose(2, 0, 1), m.spec.end_id, cons.stride, None, (cons.idf.keys, cons.idf.g),
                          cons.idf.log_ref_len)
    _check(u, b, dict(util=ru, best=rb))
    # the attention maps are the consensus-best sample's, not the likeliest sample's
    np.testing.assert_array_equal(raw['predicted_ids'].transpose(1, 2, 0), out['ids'])
    T = raw['predicted_ids'].shape[0]
    hist = raw['attn_hist'].reshape(T, B, 4, m.spec.H, m.spec.M)
    np.testing.assert_array_equal(attn, hist[:, np.arange(B), b].transpose(1, 2, 0, 3))
    likeliest = np.argmax(out['log_probs'], axis=1)
    print('consensus-best slots %r, likeliest slots %r' % (b.tolist(), likeliest.tolist()))


def test_infer_cli_writes_the_consensus_best_into_a_directory_of_its_own(tiny_run):  # noqa: F811
    ds, run_dir, ckpt = tiny_run
    num = os.path.basename(ckpt)[len('model_compact-'):-len('.npz')]
    df = _df_pickle(ds)
    common = ['--infer_checkpoints_dir', run_dir, '--dataset_dir', ds, '--infer_set', 'test', '--batch_size_infer', '2',
              '--get_metric_score', '', '--infer_checkpoints', num, '--infer_beam_size', '4']
    sampled = common + ['--infer_sample', '--infer_temperature', '1.5']
    infer = os.path.join(ROOT, 'src', 'infer.py')
    _run(infer, sampled + ['--infer_consensus', '--infer_consensus_df', df])
    out_dir = os.path.join(run_dir, 'infer_test_beam_4_lpen_0.0_smp_t1.5_s0_cns_df')
    assert not os.path.exists(os.path.join(run_dir, 'infer_test_beam_4_lpen_0.0_smp_t1.5_s0'))
    caps = json.load(open(os.path.join(out_dir, 'captions___%s.json' % num)))
    samples = json.load(open(os.path.join(out_dir, 'caption_samples___%s.json' % num)))
    assert len(caps) == 4 and len(samples) == 4
    for cap, s in zip(caps, samples):
        assert s['image_id'] == cap['image_id'] and len(s['captions']) == 4
        cns = [x['consensus'] for x in s['captions']]
        assert all(np.isfinite(v) and v >= 0.0 for v in cns)
        assert s['captions'][int(np.argmax(cns))]['caption'] == cap['caption']      # the consensus-best sample is THE caption
    with pytest.raises(ValueError, match='infer_sample'):
        _run(infer, common + ['--infer_consensus'])
