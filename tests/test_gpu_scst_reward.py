"""The SCST reward on the GPU: the operator (comic_scst_reward) and the coefficient kernel (comic_scst_coefficients)
against the float64 reference of tests/scst_reward_ref.py, the update with device rewards against the update with the same
rewards as numpy, one SCST step per mode through train_fn.scst_step on the tiny dataset, and `train.py`'s flags.

Bounds.  cider / bleu / reward / baseline within 1e-10 absolute of the reference: the bound tests/test_gpu_consensus.py
derives for the same arithmetic (at most 4 * 64 products per pair, a few ulp each on values <= 10, plus the device's exp);
BLEU's pow and exp add ulps on values <= 1.  advantage within one float32 ulp of float32(reference): the float64 difference
is within 2e-10 of the reference's, so its float32 rounding is the reference's or a neighbour.  Two launches: equal bits."""
import functools
import glob
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import comic_amd._lib as L
from comic_amd import decoder as cdec
from comic_amd.decoder import NgramIdf, Reward, RewardRefs, RewardVocab
from tests import scst_reward_ref as rr
from tests.gpu_util import DEV, dev, stream, sync
from tests.test_scst_reward_cpu import REF_LEN, WEIGHTS, make_case, on_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
MODES = {'none': rr.NONE, 'greedy': rr.ROW, 'mean': rr.LEAVE_ONE_OUT}
# (tokens, T, W, R, B[, alphabet]): the shapes of the issue -- (V, T, W, R, B) = (12, 12, 7, 5, 5), (12, 12, 2, 1, 1),
# (6, 16, 32, 5, 2) (run as an alphabet of 4 words inside the 12-entry vocabulary, so V is 12, not 6: what the small V is
# for, n-grams that repeat among the most rollouts, it keeps), (12, 1, 3, 2, 2) -- and the two radix geometries
SHAPES = [('word', 12, 7, 5, 5), ('word', 12, 2, 1, 1), ('word', 16, 32, 5, 2, 0, 4), ('word', 1, 3, 2, 2),
          ('radix4', 16, 5, 5, 3), ('radix3', 17, 4, 3, 3)]
# (..., seed, alphabet, T0): a baseline row shorter and longer than the rollouts -- the row's offset behind the [T][W]
# slice of the staged ids, Ucap taken from T0 (30 words against 9), and a radix row of an odd length
ROW_SHAPES = [('word', 12, 4, 2, 3, 0, 8, 5), ('word', 9, 3, 2, 2, 0, 8, 30), ('radix4', 12, 3, 2, 2, 0, 8, 21)]


def ulp32(x):
    return np.spacing(np.maximum(np.abs(np.asarray(x, np.float32)), np.float32(1e-30)))


@functools.lru_cache(maxsize=None)
def prepared(shape, wrap=False):
    """The case, its vocabulary, packed references, table and the reference's df on word ids, built once."""
    case = make_case(*shape)
    vocab, ref_ids, df_ids = on_ids(case)
    packed = RewardRefs.pack(case.refs, vocab)
    if not wrap:
        idf = Reward.from_pickle(case.df, case.cfg).idf
        return case, vocab, ref_ids, df_ids, packed, idf
    # a table of the minimum capacity 8 whose four entries share the last home slot: every probe sequence wraps
    grams = {}
    for rl in ref_ids:
        for r in rl:
            for ng in rr.cook(r):
                grams.setdefault(rr.ngram_key(ng), ng)
    pick = sorted((k for k in grams if k & 7 == 7), key=lambda k: (len(grams[k]), k))[:4]
    assert len(pick) == 4
    keys, g = np.zeros(8, np.uint64), np.zeros(8)
    df_wrap = {}
    for n, k in enumerate(pick):
        at = 7
        while keys[at]:
            at = (at + 1) & 7
        keys[at], g[at] = k, math.log(float(REF_LEN)) - math.log(2.0 + n)
        df_wrap[grams[k]] = 2.0 + n
    assert all(keys[s] != 0 for s in (7, 0, 1, 2))
    return case, vocab, ref_ids, df_wrap, packed, NgramIdf(keys, g, math.log(float(REF_LEN)), 1)


@functools.lru_cache(maxsize=None)
def reference(shape, weights, mode, wrap=False):
    case, vocab, ref_ids, df_ids, _, _ = prepared(shape, wrap)
    w_c, w_b = WEIGHTS[weights]
    return rr.score_ids(case.ids, ref_ids, vocab, df_ids, REF_LEN, w_c, w_b, MODES[mode],
                        case.base_ids if mode == 'greedy' else None)


def run_operator(shape, weights, mode, wrap=False):
    case, vocab, _, _, packed, idf = prepared(shape, wrap)
    w_c, w_b = WEIGHTS[weights]
    reward = Reward(w_c, w_b, idf, mode, vocab)
    ids = dev(case.ids)
    base = dev(case.base_ids) if mode == 'greedy' else None
    outs = [cdec.scst_reward(L.load(), torch, ids, packed, reward, base) for _ in range(2)]
    sync()
    return [{k: v.cpu().numpy() for k, v in o.items()} for o in outs]


def check_against_reference(got, again, want):
    for k in ('cider', 'bleu', 'reward', 'baseline'):
        assert got[k].shape == want[k].shape and got[k].dtype == np.float64, k
        err = float(np.abs(got[k] - want[k]).max())
        print('%s: max |device - reference| = %.3e' % (k, err))
        assert err <= TOL, (k, err)
    assert got['advantage'].shape == want['advantage'].shape and got['advantage'].dtype == np.float32
    assert (np.abs(got['advantage'] - want['advantage']) <= ulp32(want['advantage'])).all()
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k            # two launches, equal bits


# ---- the operator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('shape', SHAPES)
def test_operator_equals_the_reference(shape, mode):
    got, again = run_operator(shape, 'default', mode)
    check_against_reference(got, again, reference(shape, 'default', mode))
    if mode == 'mean':
        r = got['reward']
        assert (np.abs(got['advantage'].astype(np.float64).sum(axis=0)) <= 1e-5 * max(1e-30, np.abs(r).max()) + 1e-30).all()


@pytest.mark.parametrize('shape', ROW_SHAPES)
def test_operator_with_a_baseline_row_of_another_length(shape):
    assert prepared(shape)[0].base_ids.shape[0] == shape[7] != shape[1]
    got, again = run_operator(shape, 'default', 'greedy')
    check_against_reference(got, again, reference(shape, 'default', 'greedy'))
    assert np.abs(got['reward'][:, -1]).max() > 0                 # the row scores


@pytest.mark.parametrize('first_eos', [[3, 6, 1], [30, 2, 2], [0, 0, 0], [-1, -1, -1]])
def test_operator_reads_the_executed_rows_of_the_baseline_alone(first_eos):
    """baseline_first_eos: the rows behind max + 1 (never written by the greedy loop: here they hold words that would
    score) are not read; a value beyond T0 reads all rows, none executed reads none."""
    shape = ROW_SHAPES[0]                                         # T0 = 5, B = 3
    case, vocab, ref_ids, df_ids, packed, idf = prepared(shape)
    reward = Reward(1.0, (0, 0, 0, 2), idf, 'greedy', vocab)
    feos = np.array(first_eos, np.int32)
    outs = [cdec.scst_reward(L.load(), torch, dev(case.ids), packed, reward, dev(case.base_ids), dev(feos)) for _ in range(2)]
    got, again = [{k: v.cpu().numpy() for k, v in o.items()} for o in outs]
    want = rr.score_ids(case.ids, ref_ids, vocab, df_ids, REF_LEN, 1.0, (0, 0, 0, 2), rr.ROW, case.base_ids,
                        baseline_first_eos=feos)
    check_against_reference(got, again, want)
    full = reference(shape, 'default', 'greedy')
    if max(first_eos) + 1 >= 5:
        assert np.abs(want['reward'] - full['reward']).max() == 0.0
    else:
        assert np.abs(want['reward'][:, -1] - full['reward'][:, -1]).max() > 0


@pytest.mark.parametrize('weights', ['cider', 'bleu'])
def test_operator_with_one_metric_skips_the_other(weights):
    got, again = run_operator(SHAPES[0], weights, 'greedy')
    check_against_reference(got, again, reference(SHAPES[0], weights, 'greedy'))
    assert (got['bleu' if weights == 'cider' else 'cider'] == 0.0).all() and np.abs(got['reward']).max() > 0.1


@pytest.mark.parametrize('mode', ['greedy', 'mean'])
def test_operator_with_a_table_whose_probes_wrap(mode):
    got, again = run_operator(SHAPES[0], 'default', mode, wrap=True)
    want = reference(SHAPES[0], 'default', mode, wrap=True)
    check_against_reference(got, again, want)
    plain = reference(SHAPES[0], 'default', mode)
    assert np.abs(want['cider'] - plain['cider']).max() > 1e-3       # the table matters


def test_operator_without_a_table_and_through_the_decoder_method_inputs():
    """No table: every n-gram weighs 1.  numpy inputs go through the same conversion Decoder.scst_reward applies."""
    shape = SHAPES[4]
    case, vocab, ref_ids, _, packed, _ = prepared(shape)
    reward = Reward(1.0, (0, 0, 0, 2), None, 'mean', vocab)
    got = cdec.scst_reward(L.load(), torch, dev(case.ids), packed, reward)
    want = rr.score_ids(case.ids, ref_ids, vocab, None, REF_LEN, 1.0, (0, 0, 0, 2), rr.LEAVE_ONE_OUT)
    for k in ('cider', 'bleu', 'reward', 'baseline'):
        assert np.abs(got[k].cpu().numpy() - want[k]).max() <= TOL, k
    with pytest.raises(ValueError, match='beam'):
        cdec.scst_reward(L.load(), torch, dev(case.ids[:, :, :1]), packed, reward)
    with pytest.raises(ValueError, match='batch'):
        cdec.scst_reward(L.load(), torch, dev(case.ids[:, :1]), packed, reward)


# ---- the coefficients ---------------------------------------------------------------------------------------------------------
def test_coefficients_are_bit_equal_to_numpy():
    rng = np.random.default_rng(5)
    Bp, T = 6, 5
    lens = [5, 3, 0, 1, 4, 2]                                    # a row of zero length included
    wmask = (np.arange(T)[None, :] < np.array(lens)[:, None]).astype(np.float32)
    adv = (rng.standard_normal(Bp) * 3).astype(np.float32)
    coef, rs = torch.empty((Bp, T), device=DEV), torch.empty((Bp, T), device=DEV)
    wm, ad = dev(wmask), dev(adv)
    L.check(L.load().comic_scst_coefficients(wm.data_ptr(), ad.data_ptr(), Bp, T, coef.data_ptr(), rs.data_ptr(), stream()),
            'scst_coefficients')
    sync()
    want_coef, want_rs = rr.coefficients(wmask, adv)
    assert coef.cpu().numpy().tobytes() == want_coef.tobytes()
    assert rs.cpu().numpy().tobytes() == want_rs.tobytes()


# ---- the update ---------------------------------------------------------------------------------------------------------------
def test_update_with_device_rewards_equals_the_update_with_numpy_rewards():
    from tests.test_gpu_ensemble import _rand_params, _spec_and_cfg
    spec, cfg = _spec_and_cfg()
    p = _rand_params(cfg, 3, 1.0)
    rng = np.random.default_rng(11)
    B, Lc = 6, 9
    caps = np.full((B, Lc), -1, np.int64)
    for b in range(B):
        n = int(rng.integers(1, Lc - 1))
        caps[b, 0] = spec.start_id
        caps[b, 1:1 + n] = rng.integers(0, 200, n)
        caps[b, 1 + n] = spec.end_id
    fm = dev(rng.standard_normal((B, spec.M, spec.C)).astype(np.float32))
    im = dev(rng.standard_normal((B, spec.Cg)).astype(np.float32))
    rewards = (rng.standard_normal(B) * 2).astype(np.float32)

    def run(rw, split):
        dec = cdec.Decoder(spec, p, DEV)
        if split:
            dec.train_step(fm, im, caps, training=True, seed=77, phase='fwd')
            res = dec.train_step(None, None, caps, rewards=rw, training=True, phase='bwd')
        else:
            res = dec.train_step(fm, im, caps, rewards=rw, training=True, seed=77)
        sync()
        return np.float32(float(res['loss'])).tobytes(), dec.grads.data.cpu().numpy().tobytes()
    for split in (False, True):
        host = run(rewards, split)
        device = run(dev(rewards), split)
        assert host[0] == device[0], 'loss, split=%r' % split
        assert host[1] == device[1], 'gradients, split=%r' % split
    assert run(rewards, False) == run(rewards, True)
    dec = cdec.Decoder(spec, p, DEV)
    with pytest.raises(ValueError, match='device rewards'):
        dec.train_step(fm, im, caps, rewards=dev(rewards.astype(np.float64)), training=True, seed=77)


# ---- the loop -------------------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location('cli_train_scst_reward', os.path.join(ROOT, 'src', 'train.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TINY = ['--cnn_name', 'inception_v3', '--cnn_fm_attention', 'Mixed_7c', '--cnn_input_size', '139,139', '--batch_size_eval', '4',
        '--rnn_size', '128', '--rnn_word_size', '64']


@pytest.fixture(scope='module')
def scst_runs(tmp_path_factory):
    """One SCST step per mode on the tiny dataset, driven as `try_to_train(train_fn=probe)` drives the loop: freshly
    initialised models (the same seed every time) and the first batches of the same input manager settings."""
    from tests import tiny_dataset
    from comic_amd import inputs, model as mdl, train_fn as train
    from comic_amd.scst.scorers import captionScorer
    tmp = tmp_path_factory.mktemp('scst_reward')
    ds = tiny_dataset.make(str(tmp / 'mscoco'), n_train=16, n_valid=4, n_test=4)
    cli = _cli()
    runs = {}

    def probe(config, name, steps):
        mdl.reset_default_graph()
        man = inputs.InputManager_SCST(config)
        try:
            man.enable_device_preprocess(DEV)
            c = man.config
            m_train = mdl.CaptionModel_SCST(c, scst_mode='train', reuse=False, device=DEV)
            m_sample = mdl.CaptionModel_SCST(c, scst_mode='sample', reuse=True, device=DEV)
            # a freshly initialised decoder spells almost no word of the 20-word vocabulary (every reward would be that of
            # an empty caption): lift the 20 words' output biases, and <EOS> enough for samples to end
            b_o = m_train.decoder.params.view('b_o')
            b_o[:20] += 6.0
            b_o[c.radix_base + 1] += 5.0
            idf_fp = os.path.join(c.dataset_dir, 'captions', c.dataset_file_pattern.format('scst-words') + '.p')
            scorer = captionScorer(idf_fp, dict(ciderD=c.scst_weight_ciderD, bleu=c.scst_weight_bleu))
            o = train.scst_options(c)
            reward = Reward.from_pickle(idf_fp, c, baseline=o.baseline) if o.reward == 'device' else None
            out, seen = [], []
            dec, ids_of = m_sample.decoder, m_sample.decoder.beam_search_ids

            def spy(*a, **kw):                   # what sample() hands the rollouts: (global step, image_base)
                seen.append((m_train.global_step, kw.get('image_base', 0)))
                return ids_of(*a, **kw)
            if o.rollout == 'sample':
                dec.beam_search_ids = spy
            for _ in range(steps):
                imgs, refs = next(man.batch_train)
                res = train.scst_step(c, man, m_sample, m_train, scorer, imgs, refs, reward=reward)
                rw = res.rewards
                full = None
                if torch.is_tensor(rw):
                    full = res.reward_device['reward'].cpu().numpy()
                    rw = rw.cpu().numpy().reshape(-1)
                out.append(dict(ids=np.asarray(res.ids).copy(), adv=np.asarray(rw).copy(), reward=full, ppl=float(res.ppl)))
            if name == 'sampled_a':
                # rank 1 of 2 at this global step, on the images of the last step; then the noise itself: the same
                # features under the same base, and under the base of the next batch
                from types import SimpleNamespace
                own, m_sample.dp = m_sample.dp, SimpleNamespace(world=2, rank=1)
                m_sample.sample(imgs, rollout='sample', greedy=False)
                m_sample.dp = own
                rng = np.random.default_rng(3)
                s = dec.spec
                fm, im = dev(rng.standard_normal((10, s.M, s.C)).astype(np.float32)), dev(rng.standard_normal((10, s.Cg)).astype(np.float32))
                smp = cdec.BeamSampling(1.0, seed=int(c.rand_seed))
                runs['noise'] = [ids_of(fm, im, 3, 20, sampling=smp, image_base=b)() for b in (0, 0, 10)]
            torch.cuda.synchronize()
            runs[name], runs[name + '_bases'] = out, seen
        finally:
            man.close()
    for name, extra, steps in (('host', [], 1), ('device', ['--scst_reward', 'device'], 1),
                               ('sampled_a', ['--scst_rollout', 'sample', '--scst_baseline', 'mean', '--scst_reward', 'device'], 2),
                               ('sampled_b', ['--scst_rollout', 'sample', '--scst_baseline', 'mean', '--scst_reward', 'device'], 2)):
        logs = str(tmp / ('experiments_' + name))               # a root of its own: where the reward is formed changes no name
        os.makedirs(os.path.join(logs, 'mscoco', 'radix_b256_add_LN_softmax_h8_tie_lstm_cnnFT_run_01'))
        args = ['--dataset_dir', ds, '--log_root', logs] + TINY + ['--train_mode', 'scst', '--scst_beam_size', '3'] + extra
        kwargs, _, overwrite = cli.build_kwargs(cli.create_parser().parse_args(args))
        train.try_to_train(train_fn=lambda cfg: probe(cfg, name, steps), try_block=False, overwrite=overwrite, **kwargs)
    return runs


def test_loop_host_and_device_rewards_agree(scst_runs):
    """Beam rollouts and the greedy baseline: the advantage the update takes, formed by the host scorer on text and by the
    device launch on ids, within one float32 ulp."""
    h, d = scst_runs['host'][0], scst_runs['device'][0]
    np.testing.assert_array_equal(h['ids'], d['ids'])
    want = h['adv'].astype(np.float32)
    assert d['adv'].dtype == np.float32 and d['adv'].shape == want.shape == (3 * 10,)
    print('advantage: max |host| %.3e, max |device - host| %.3e' % (np.abs(want).max(), np.abs(d['adv'] - want).max()))
    assert (np.abs(d['adv'] - want) <= ulp32(want)).all(), np.abs(d['adv'] - want).max()
    assert np.abs(want).max() > 1e-3                              # rollouts that score: the comparison is not 0 against 0
    assert np.isfinite(h['ppl']) and np.isfinite(d['ppl'])


def test_loop_sampled_rollouts_with_the_mean_baseline(scst_runs):
    a, b = scst_runs['sampled_a'], scst_runs['sampled_b']
    for x, y in zip(a, b):                                       # the same seed: the same ids and advantages
        np.testing.assert_array_equal(x['ids'], y['ids'])
        assert x['adv'].tobytes() == y['adv'].tobytes()
    assert a[0]['ids'].shape != a[1]['ids'].shape or (a[0]['ids'] != a[1]['ids']).any()      # the steps differ
    # image_base = (global step * world + rank) * batch: steps 0 and 1 of one process, then rank 1 of 2 at step 2
    assert scst_runs['sampled_a_bases'] == [(0, 0), (1, 10), (2, (2 * 2 + 1) * 10)]
    assert scst_runs['sampled_b_bases'] == [(0, 0), (1, 10)]
    same, again, moved = scst_runs['noise']                      # ... and the base is what moves the noise
    np.testing.assert_array_equal(same, again)
    assert same.shape != moved.shape or (same != moved).any()
    for x in a:
        adv = x['adv'].astype(np.float64).reshape(3, 10)
        assert (np.abs(adv.sum(axis=0)) <= 1e-5 * np.abs(x['reward']).max()).all()
        print('sampled step: max |reward| %.3e, max |advantage| %.3e' % (np.abs(x['reward']).max(), np.abs(adv).max()))
        assert np.abs(adv).max() > 1e-3
        assert np.isfinite(x['ppl'])


# ---- the CLI ------------------------------------------------------------------------------------------------------------------
def test_cli_scst_with_sampled_rollouts_mean_baseline_and_device_rewards(tmp_path):
    from tests import tiny_dataset
    from comic_amd import configuration as conf
    ds = tiny_dataset.make(str(tmp_path / 'mscoco'), n_train=16, n_valid=4, n_test=4)
    logs = str(tmp_path / 'experiments')
    common = ['--dataset_dir', ds, '--log_root', logs] + TINY
    cli = _cli()
    cli.main(common + ['--train_mode', 'decoder', '--batch_size_train', '8', '--max_epoch', '1'])
    cli.main(common + ['--train_mode', 'cnn_finetune', '--batch_size_train', '8', '--max_epoch', '1'])
    cli.main(common + ['--train_mode', 'scst', '--max_epoch', '1', '--scst_rollout', 'sample', '--scst_baseline', 'mean',
                       '--scst_reward', 'device', '--scst_beam_size', '3'])
    errs = glob.glob(os.path.join(logs, 'mscoco', 'error__*'))
    assert not errs, open(errs[0]).read()
    dirs = glob.glob(os.path.join(logs, 'mscoco', '*_SCST_beam_3_*_smp_loo_*'))
    assert dirs and glob.glob(os.path.join(dirs[0], 'model_compact-*.npz'))
    c = conf.load_config(os.path.join(dirs[0], 'config.pkl'))
    assert (c.scst_rollout, c.scst_baseline, c.scst_reward, c.scst_temperature) == ('sample', 'mean', 'device', 1.0)
