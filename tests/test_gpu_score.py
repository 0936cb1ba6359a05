"""Caption scoring (comic_decoder_score / Decoder.score / CaptionModel.score_captions) against the CPU oracle's
teacher-forced logits (oracle/decoder_ref.py), turned into log_softmax and gathered at the targets here."""
import numpy as np
import pytest
import torch

from comic_amd import decoder as cdec
from oracle import decoder_ref as dr
from tests import exec_ops_ref
from tests.gpu_util import DEV, F32_RTOL, assert_close, dev, elementwise_excess, rel_err, sync
from tests.test_gpu_path import _rand_params, _spec_and_cfg

pytestmark = pytest.mark.gpu

CHUNK = 112                      # vocabulary columns of a workgroup of the streaming projection (csrc/beam_pack.h)
# Largest |score - log_softmax(train_step logits)[target]| / max|log p| measured over the cases of CASES on an MI355X:
# see test_score_agrees_with_the_materialised_path.
MATERIALISED_MEASURED = 1.7e-7
MATERIALISED_BAR = 4 * MATERIALISED_MEASURED


def _log_softmax_at(logits, targets, wmask):
    """[B,T,V] float -> log_softmax gathered at targets [B,T], times the mask, in float64."""
    x = np.asarray(logits, np.float64)
    m = x.max(axis=-1, keepdims=True)
    lse = m[..., 0] + np.log(np.exp(x - m).sum(axis=-1))
    return (np.take_along_axis(x, targets[..., None].astype(np.int64), -1)[..., 0] - lse) * wmask


def _caps(spec, B, L, seed, lens=None, place=()):
    """Captions [B,L] (PAD = -1): row 0 fills L, other rows ragged (or `lens` tokens + EOS); `place`: (row, position, id) of
    target columns put there on purpose."""
    rng = np.random.default_rng(seed)
    caps = np.full((B, L), -1, np.int64)
    for b in range(B):
        n = (L - 2 if b == 0 else int(rng.integers(1, L - 1))) if lens is None else lens[b]
        caps[b, 0] = spec.start_id
        caps[b, 1:1 + n] = rng.integers(0, spec.V - 2, n)
        caps[b, 1 + n] = spec.end_id
    for b, i, v in place:
        caps[b, 1 + i] = v
    return caps


def _features(spec, B, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, spec.M, spec.C)).astype(np.float32), rng.standard_normal((B, spec.Cg)).astype(np.float32))


_BIG = dict(D=512, E=256, C=2048, Cg=2048)
_WORD = dict(token_type='word', V=4099, start_id=4097, end_id=4098)
CASES = {
    # small vocabulary, persistent forward loop: one caption with a single token (EOS alone), one that fills T
    'small': dict(kw=_BIG, B=3, L=9, lens=[7, 0, 3], place=(), path=1),
    # large vocabulary, rows below one 16-row tile (persistent loop, four K-quarters)
    'large_tile': dict(kw=dict(_BIG, **_WORD), B=2, L=4, lens=[2, 1], place=((0, 0, CHUNK - 1), (0, 1, CHUNK), (1, 0, 0)), path=3),
    # large vocabulary, 296 rows: across a 256-row block and no multiple of 16 (per-step forward, two K-quarters)
    'large_block': dict(kw=dict(D=256, E=64, **_WORD), B=37, L=9, lens=None,
                        place=((0, 0, 0), (0, 1, CHUNK - 1), (0, 2, CHUNK), (0, 3, 4096), (0, 4, 4095), (1, 0, 2 * CHUNK - 1)), path=2),
}
_cache = {}


def _case(name):
    """Oracle reference and device results of a case, computed once and shared (left unchanged by the tests)."""
    if name in _cache:
        return _cache[name]
    c = CASES[name]
    spec, cfg = _spec_and_cfg(**c['kw'])
    p = _rand_params(cfg, 3)
    fm, im = _features(spec, c['B'], 7)
    caps = _caps(spec, c['B'], c['L'], 11, c['lens'], c['place'])
    _, targets, wmask, lens = dr.process_inputs(caps, cfg.token_type)
    cfg.l2_decay = 0.0
    out = dr.train_forward(p, cfg, fm, im, caps, None, None)
    want = _log_softmax_at(out['logits'], targets, wmask)
    dec = cdec.Decoder(spec, p, DEV)
    res = dec.score(dev(fm), dev(im), caps, want_attention=True)
    sync()
    r = dict(spec=spec, cfg=cfg, p=p, fm=fm, im=im, caps=caps, targets=targets, wmask=wmask, lens=lens, want=want, dec=dec,
             path=dec.lib.comic_decoder_score_path(), tok=res['token_log_probs'].cpu().numpy().copy(),
             logp=res['log_prob'].cpu().numpy().copy(), maps=res['attn_maps'].cpu().numpy().copy(), out=out)
    _cache[name] = r
    return r


@pytest.mark.parametrize('name', list(CASES))
def test_score_matches_oracle(name):
    """Token and caption log-probs against the oracle at the bar of the logits comparisons (F32_RTOL, max-norm relative to
    max |log p|, and element-wise), on the path the case is meant for; targets at column 0, V - 1 (= end_id), the last
    column of chunk 0, the first of chunk 1 and in the ragged last chunk."""
    r = _case(name)
    assert r['path'] == CASES[name]['path']
    if CASES[name]['place']:
        live = r['targets'][r['wmask'] > 0]
        for v in [v for _, _, v in CASES[name]['place']] + [r['spec'].V - 1]:
            assert v in live, v
    print('%s: token rel err %.3e, caption rel err %.3e' % (name, rel_err(r['tok'], r['want']),
                                                           rel_err(r['logp'], r['want'].sum(axis=1))))
    assert_close(r['tok'], r['want'], F32_RTOL, 'token log-probs')
    assert_close(r['logp'], r['want'].sum(axis=1), F32_RTOL, 'caption log-probs')
    assert_close(r['maps'], r['out']['attn_maps'], F32_RTOL, 'attention maps')
    np.testing.assert_array_equal(r['lens'], np.asarray(r['dec'].score(dev(r['fm']), dev(r['im']), r['caps'])['lengths']))


@pytest.mark.parametrize('name', list(CASES))
def test_score_agrees_with_the_materialised_path(name):
    """Against log_softmax(train_step(training=False)['logits']) of the same library.  Measured on an MI355X over the three
    cases (max-norm relative to max |log p|): small 1.09e-7, large_tile 9.5e-8, large_block 1.62e-7 (the same figures in every run:
    both sides are deterministic); the bar is four times the largest, rounded up to 1.7e-7, and far below the oracle bar."""
    r = _case(name)
    dec = cdec.Decoder(r['spec'], r['p'], DEV)
    res = dec.train_step(dev(r['fm']), dev(r['im']), r['caps'], training=False)
    sync()
    want = _log_softmax_at(res['logits'].cpu().numpy(), r['targets'], r['wmask'])
    e = rel_err(r['tok'], want)
    print('%s: score vs materialised logits: %.3e' % (name, e))
    assert MATERIALISED_BAR < F32_RTOL
    assert e <= MATERIALISED_BAR, e


@pytest.mark.parametrize('name', list(CASES))
def test_masking_and_order(name):
    """wmask == 0 -> exactly 0.0; log_prob[b] = float32 sum of the row's tokens in t order, bit for bit."""
    r = _case(name)
    assert (r['tok'][r['wmask'] == 0] == 0.0).all() and not np.signbit(r['tok'][r['wmask'] == 0]).any()
    assert (r['tok'][r['wmask'] > 0] < 0.0).all()
    for b in range(r['tok'].shape[0]):
        acc = np.float32(0.0)
        for t in range(r['tok'].shape[1]):
            acc = np.float32(acc + r['tok'][b, t])
        assert acc.tobytes() == r['logp'][b].tobytes(), b


@pytest.mark.parametrize('name', list(CASES))
def test_score_is_deterministic_and_moves_nothing_else(name):
    """Two more calls: the bits of the first.  The gradient buffer (sentinel-filled) and the parameters are untouched."""
    r = _case(name)
    dec = r['dec']
    dec.grads.data.fill_(-123.5)
    before = dec.params.data.clone()
    for _ in range(2):
        res = dec.score(dev(r['fm']), dev(r['im']), r['caps'])
        sync()
        assert np.array_equal(res['token_log_probs'].cpu().numpy(), r['tok'])
        assert np.array_equal(res['log_prob'].cpu().numpy(), r['logp'])
    assert bool((dec.grads.data == -123.5).all())
    assert torch.equal(dec.params.data, before)


@pytest.mark.parametrize('kw,env', [(dict(_BIG), {'COMIC_PERSIST': '0'}), (dict(rnn_name='LN_LSTM'), {}), (dict(rnn_name='GRU'), {})])
def test_per_step_forms(kw, env, monkeypatch):
    """COMIC_DEC_NO_PERSIST with the LSTM, and the LN_LSTM / GRU cells (per-step launches), at B = 2, V = 258."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    spec, cfg = _spec_and_cfg(**kw)
    p = _rand_params(cfg, 5)
    fm, im = _features(spec, 2, 9)
    caps = _caps(spec, 2, 8, 13, [6, 2])
    _, targets, wmask, _ = dr.process_inputs(caps, cfg.token_type)
    out = dr.train_forward(p, cfg, fm, im, caps, None, None)
    want = _log_softmax_at(out['logits'], targets, wmask)
    dec = cdec.Decoder(spec, p, DEV)
    res = dec.score(dev(fm), dev(im), caps)
    sync()
    assert dec.lib.comic_decoder_score_path() & 1 == 0
    assert_close(res['token_log_probs'].cpu().numpy(), want, F32_RTOL, 'token log-probs')
    assert_close(res['log_prob'].cpu().numpy(), want.sum(axis=1), F32_RTOL, 'caption log-probs')


# per-step launches and the persistent forward loop at V = 258 (one partial per row: score_rows_kernel, the merge loop of
# score_merge_kernel runs once), and V = 4099: 37 chunk partials per row, the chunk merge proper (path 3, as `large_tile`)
@pytest.mark.parametrize('name,env,path', [('V258', {'COMIC_PERSIST': '0'}, 0), ('V258', {}, 1), ('V4099', {}, 3)],
                         ids=['per_step_V258', 'persistent_V258', 'chunk_merge_V4099'])
def test_score_peaked_logits(name, env, path, monkeypatch):
    """The regime `peaked` of tests/regimes.py through the output projection, against the oracle in float64: W_o scaled so
    that the logits spread like 30 N(0,1), b_o + 200 (expf overflows without the max subtraction; a chunk partial's
    exp(pmax - mx) underflows for most chunks).  Token log-probs reach -150 and further, so they are held element-wise
    beside the max-norm, at the bar of test_per_step_forms.  The operands are exec_ops_ref.score_peaked_case, on which
    tests/test_regimes_cpu.py holds the float32 oracle below a tenth of the bar."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = exec_ops_ref.score_peaked_case(name)
    spec, _ = _spec_and_cfg(**exec_ops_ref.SCORE_PEAKED_GEOMETRIES[name])
    cfg, p, fm, im, caps, out = (c[k] for k in ('cfg', 'p', 'fm', 'im', 'caps', 'out'))
    _, targets, wmask, _ = dr.process_inputs(caps, cfg.token_type)
    want = _log_softmax_at(out['logits'], targets, wmask)
    assert np.abs(out['logits']).max() > 250 and want.min() < -100
    dec = cdec.Decoder(spec, p, DEV)
    res = dec.score(dev(fm), dev(im), caps)
    sync()
    assert dec.lib.comic_decoder_score_path() == path         # 3: the streaming projection and its 37-chunk merge really ran
    tok, logp = res['token_log_probs'].cpu().numpy(), res['log_prob'].cpu().numpy()
    print('  V=%d: token log-probs %.1f ... %.1f, err %.3e  element-wise %.3e  bar %.1e' % (
        spec.V, want.min(), want[wmask > 0].max(), rel_err(tok, want), elementwise_excess(tok, want, 1.0), F32_RTOL))
    assert_close(tok, want, F32_RTOL, 'token log-probs')
    assert_close(logp, want.sum(axis=1), F32_RTOL, 'caption log-probs')


@pytest.mark.parametrize('name', ['small', 'large_block'])
def test_graph_replay_equals_eager(name):
    """use_graph: call 1 eager, call 2 captures, call 3 replays -- on new captions of the same shape, the eager bits."""
    r = _case(name)
    c = CASES[name]
    a, b = cdec.Decoder(r['spec'], r['p'], DEV), cdec.Decoder(r['spec'], r['p'], DEV)
    lens = r['lens'] - 1
    for it in range(3):
        caps = _caps(r['spec'], c['B'], c['L'], 100 + it, list(lens))
        fm, im = _features(r['spec'], c['B'], 200 + it)
        ra = a.score(dev(fm), dev(im), caps, use_graph=False)
        rb = b.score(dev(fm), dev(im), caps, use_graph=True)
        sync()
        assert torch.equal(ra['token_log_probs'], rb['token_log_probs']), it
        assert torch.equal(ra['log_prob'], rb['log_prob']), it
    assert b._score_ctxs[(c['B'], c['L'] - 1, int(r['lens'].max()), False)].graph is not None


def test_workspace_holds_no_logits_block():
    """V = 25 599, B = 64, T = 20: the scoring workspace is smaller than the training one by more than the [T,B,V] d-logits
    block, and smaller than one such block plus the forward's buffers would be."""
    spec, _ = _spec_and_cfg(**dict(_BIG, token_type='word', V=25599, start_id=25597, end_id=25598))
    import ctypes as C
    lib = cdec.L.load()
    d = spec.desc(False)
    train, score = lib.comic_decoder_train_workspace(C.byref(d), 64, 20), lib.comic_decoder_score_workspace(C.byref(d), 64, 20)
    print('workspace bytes at V = 25599, B = 64, T = 20: train %d, score %d' % (train, score))
    block = 64 * 20 * 25599 * 4
    assert 0 < score < train - block


def test_end_to_end_model_scores_its_own_greedy_output(tmp_path):
    """CaptionModel from the CLI's configuration on a tiny dataset: greedy(want_logits=True) for 2 images, then
    score_captions(images, greedy ids): teacher-forcing the model's own output reproduces its states, so the token
    log-probs equal log_softmax(greedy logits) at the chosen ids.  run_eval_step(forward_only=True) equals run_eval_step()."""
    import importlib.util
    import os
    from tests import tiny_dataset
    from comic_amd import model as mdl, train_fn as train
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ds = tiny_dataset.make(str(tmp_path / 'mscoco'), n_train=8, n_valid=4, n_test=4)
    sp = importlib.util.spec_from_file_location('cli_train_score', os.path.join(root, 'src', 'train.py'))
    cli = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(cli)
    args = cli.create_parser().parse_args(
        ['--dataset_dir', ds, '--log_root', str(tmp_path / 'experiments'), '--cnn_name', 'inception_v3',
         '--cnn_fm_attention', 'Mixed_7c', '--cnn_input_size', '139,139', '--batch_size_eval', '4', '--rnn_size', '128',
         '--rnn_word_size', '64', '--train_mode', 'decoder', '--batch_size_train', '2', '--max_epoch', '1'])
    kwargs, _, overwrite = cli.build_kwargs(args)
    seen = []

    def probe(config):
        mdl.reset_default_graph()
        man = train._manager(config)
        try:
            man.enable_device_preprocess('cuda:0')
            m = mdl.CaptionModel(config, mode='train', batch_ops=man.batch_train, reuse=False, name='train', device='cuda:0')
            images, gt = next(man.batch_train)
            s = m.spec
            im_embed, fm = m._encode_copy(images)
            ids, _, logits = m.decoder.greedy(fm, im_embed, 8, want_logits=True)
            sync()
            ids = np.asarray(ids)
            caps = np.full((ids.shape[0], ids.shape[1] + 1), -1, np.int64)
            caps[:, 0] = s.start_id
            for b in range(ids.shape[0]):
                row = list(ids[b])
                n = row.index(s.end_id) + 1 if s.end_id in row else len(row)
                caps[b, 1:1 + n] = row[:n]
            res = m.score_captions(images, caps)
            sync()
            _, targets, wmask, _ = dr.process_inputs(caps, s.token_type)
            want = _log_softmax_at(logits.cpu().numpy(), targets, wmask)
            assert_close(res['token_log_probs'].cpu().numpy(), want, F32_RTOL, 'token log-probs of the greedy output')
            a, b = float(m.run_eval_step((images, gt))), float(m.run_eval_step((images, gt), forward_only=True))
            assert abs(a - b) <= F32_RTOL * abs(a), (a, b)
            seen.append((a, b))
        finally:
            man.close()
    train.try_to_train(train_fn=probe, try_block=False, overwrite=overwrite, **kwargs)
    assert seen
