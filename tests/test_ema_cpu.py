"""`--ema_decay`, `--infer_ema`, `--infer_average` on the host side (no GPU): the warm-up rate, the CLI refusals, the
shadows' names and their way through both checkpoint containers, the checkpoint average."""
import importlib.util
import os

import numpy as np
import pytest

from comic_amd import checkpoint as ckpt, decoder as cdec, optim
from tests import ema_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli(name):
    spec = importlib.util.spec_from_file_location('cli_%s_ema' % name, os.path.join(ROOT, 'src', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the rate ------------------------------------------------------------------------------------------------------------
def test_ema_rate_closed_form_crossover_and_monotony():
    # t counts the updates including this one: n = t - 1, rate (1 + n) / (10 + n) while that is below the decay
    for t, want in ((1, 1 / 10), (2, 2 / 11), (9, 9 / 18), (10, 10 / 19), (11, 11 / 20)):
        assert optim.ema_rate(0.9999, t) == pytest.approx(want, rel=1e-15), t
        assert optim.ema_rate(0.9999, t) == pytest.approx(ema_ref.rate(0.9999, t), rel=1e-15)
    # decay 0.5: (1 + n) / (10 + n) reaches 0.5 at n = 8 (t = 9); from there on the fixed decay
    assert [optim.ema_rate(0.5, t) for t in (8, 9, 10, 11, 1000)] == [pytest.approx(8 / 17), 0.5, 0.5, 0.5, 0.5]
    assert optim.ema_rate(0.5, 8) < 0.5
    for decay in (0.5, 0.9, 0.999, 0.9999):
        r = [optim.ema_rate(decay, t) for t in range(1, 200001, 7)]
        assert all(b >= a for a, b in zip(r, r[1:])) and max(r) <= decay and r[0] == pytest.approx(0.1)
        assert r[-1] == decay               # (0.9999 is reached at n = 89990)


# ---- train.py ------------------------------------------------------------------------------------------------------------
def test_train_refuses_a_bad_ema_decay_before_the_gpu(tmp_path):
    mod = _cli('train')
    for bad in ('1.0', '-0.1'):
        with pytest.raises(ValueError, match='ema_decay'):
            # main() refuses right after parsing: nothing is imported from torch, no directory is created
            mod.main(['--ema_decay', bad, '--log_root', '/nonexistent/never/created'])
        with pytest.raises(ValueError, match='ema_decay'):
            mod.check_supported({'train_mode': 'decoder', 'cnn_dtype': 'bf16', 'ema_decay': float(bad)})
    assert not os.path.exists('/nonexistent/never/created')
    mod.check_supported({'train_mode': 'decoder', 'cnn_dtype': 'bf16'})             # (a configuration from before the flag)
    plain, _, _ = mod.build_kwargs(mod.create_parser().parse_args(['--log_root', str(tmp_path)]))
    zero, _, _ = mod.build_kwargs(mod.create_parser().parse_args(['--log_root', str(tmp_path), '--ema_decay', '0']))
    assert zero == plain and 'ema_decay' not in plain                               # off: the parent's kwargs
    on, _, _ = mod.build_kwargs(mod.create_parser().parse_args(['--log_root', str(tmp_path), '--ema_decay', '0.999']))
    assert on.pop('ema_decay') == 0.999 and on == plain


# ---- names and containers ------------------------------------------------------------------------------------------------
def _spec_and_arrays(seed=1):
    spec = cdec.DecoderSpec(D=16, E=8, V=20, C=12, Cg=12, H=2, M=4)
    rng = np.random.default_rng(seed)
    dec = {k: rng.standard_normal(v).astype(np.float32) for k, v in spec.param_shapes().items()}
    ema = {k: rng.standard_normal(v).astype(np.float32) for k, v in spec.param_shapes().items()}
    cnn = {'InceptionV3/Conv2d_1a_3x3/weights': rng.standard_normal((3, 3, 3, 4)).astype(np.float32),
           'InceptionV3/Conv2d_1a_3x3/BatchNorm/beta': rng.standard_normal(4).astype(np.float32)}
    return spec, dec, ema, cnn


def test_ema_tf_names_round_trip():
    spec, dec, ema, _ = _spec_and_arrays()
    tf = ckpt.ema_to_tf(spec, ema)
    assert set(tf) == {n + '/ExponentialMovingAverage' for n in ckpt.decoder_var_names(spec).values()}
    back = ckpt.ema_from_tf(spec, tf)
    assert set(back) == set(ema) and all(np.array_equal(back[k], ema[k]) for k in ema)
    one_short = dict(tf)
    one_short.pop(sorted(tf)[0])
    assert ckpt.ema_from_tf(spec, one_short) is None and ckpt.ema_from_tf(spec, {}) is None


@pytest.mark.parametrize('fmt', ['npz', 'tf'])
def test_shadows_travel_through_the_full_checkpoint(tmp_path, fmt):
    spec, dec, ema, cnn = _spec_and_arrays()
    cnn_ema = {ckpt.CNN_SCOPE + k + ckpt.EMA_SUFFIX: v + 1 for k, v in cnn.items()}
    flat = np.arange(7, dtype=np.float32)
    extra = dict(ckpt.ema_to_tf(spec, ema), **cnn_ema) if fmt == 'tf' else {'optimise/caption/ema': flat}
    path = ckpt.save(str(tmp_path / 'model'), 5, cnn, spec, dec, extra, fmt=fmt)
    c2, d2, got = ckpt.restore(path, list(cnn), spec, resume_training=True)
    # the model variables are found as before: the suffix names are slots, not variables
    assert set(c2) == set(cnn) and set(d2) == set(dec) and all(np.array_equal(d2[k], dec[k]) for k in dec)
    assert int(got['global_step']) == 5
    if fmt == 'tf':
        back = ckpt.ema_from_tf(spec, got)
        assert all(np.array_equal(back[k], ema[k]) for k in ema)
        assert all(np.array_equal(got[k], v) for k, v in cnn_ema.items())
        assert not any(k.startswith('Model/') and not k.endswith(ckpt.EMA_SUFFIX) for k in got)
    else:
        assert np.array_equal(got['optimise/caption/ema'], flat)
    c3, d3, none = ckpt.restore(path, list(cnn), spec, resume_training=False)
    assert none == {} and set(d3) == set(dec) and set(c3) == set(cnn)


# ---- the checkpoint average ----------------------------------------------------------------------------------------------
def test_average_variables():
    rng = np.random.default_rng(3)
    a = {'Model/x': rng.standard_normal((5, 7)).astype(np.float32), 'Model/y': rng.standard_normal(3).astype(np.float32),
         'global_step': np.asarray(4, np.int32)}
    for M in (1, 2, 3, 7):
        same = ckpt.average_variables([dict(a) for _ in range(M)])
        assert set(same) == set(a) and all(same[k].dtype == a[k].dtype and np.array_equal(same[k], a[k]) for k in a)
    b = {'Model/x': (1e-3 * rng.standard_normal((5, 7))).astype(np.float32),
         'Model/y': (1e3 * rng.standard_normal(3)).astype(np.float32), 'global_step': np.asarray(9, np.int32)}
    mean = ckpt.average_variables([a, b])
    for k in ('Model/x', 'Model/y'):
        want = ((a[k].astype(np.float64) + b[k].astype(np.float64)) / 2).astype(np.float32)      # rounded once
        assert mean[k].dtype == np.float32 and np.array_equal(mean[k], want)
    assert int(mean['global_step']) == 9
    c = dict(b, **{'Model/y': np.zeros(4, np.float32)})
    with pytest.raises(ValueError, match='Model/y'):
        ckpt.average_variables([a, c])
    d = {k: v for k, v in b.items() if k != 'Model/x'}
    with pytest.raises(ValueError, match='Model/x'):
        ckpt.average_variables([a, d])


# ---- infer.py / score.py -------------------------------------------------------------------------------------------------
def test_infer_ema_prefix_and_directory_suffix():
    mod = _cli('infer')
    parser = mod.create_parser()
    overlay = {k: v for k, v in parser.parse_args([]).__dict__.items() if v is not None}
    assert not {'infer_ema', 'infer_average'} & set(overlay)
    plain, ema = parser.parse_args([]), parser.parse_args(['--infer_ema'])
    assert (mod.checkpoint_prefix(plain), mod.ema_dir_suffix(plain), mod.average_dir_suffix(plain)) == ('model_compact-', '', '')
    assert (mod.checkpoint_prefix(ema), mod.ema_dir_suffix(ema)) == ('model_ema-', '_ema')
    avg = parser.parse_args(['--infer_average', '--infer_ema', '--infer_checkpoints', '4,8,12'])
    avg.infer_checkpoints = avg.infer_checkpoints.split(',')
    assert mod.ema_dir_suffix(avg) + mod.average_dir_suffix(avg) == '_ema_avg_4+8+12'


def test_infer_refuses_before_anything_is_loaded(tmp_path):
    mod = _cli('infer')
    run = str(tmp_path)                 # no config.pkl, no checkpoint: anything that loaded would fail otherwise
    with pytest.raises(ValueError, match='at least two'):
        mod.main(['--infer_checkpoints_dir', run, '--infer_average', '--infer_checkpoints', '4'])
    with pytest.raises(ValueError, match='infer_ensemble'):
        mod.main(['--infer_checkpoints_dir', run, '--infer_average', '--infer_ensemble', '--infer_checkpoints', '4,8'])
    with pytest.raises(ValueError, match='--ema_decay'):
        mod.main(['--infer_checkpoints_dir', run, '--infer_ema'])
    assert os.listdir(run) == []


def test_score_finds_the_ema_checkpoints(tmp_path):
    mod = _cli('score')
    for f in ('model_compact-4.npz', 'model_compact-8.npz', 'model_ema-4.npz', 'model_ema-8.index',
              'model_ema-8.data-00000-of-00001', 'model-8.npz', 'config.pkl'):
        open(tmp_path / f, 'w').close()
    assert mod.find_checkpoints(str(tmp_path), 'all', prefix='model_ema-') == ['4', '8']
    assert mod.find_checkpoints(str(tmp_path), 'all') == ['4', '8']
    os.remove(tmp_path / 'model_ema-4.npz')
    assert mod.find_checkpoints(str(tmp_path), 'all', prefix='model_ema-') == ['8']
    assert mod.create_parser().parse_args(['--captions_file', 'c.json', '--infer_ema']).infer_ema is True
    assert mod.create_parser().parse_args(['--captions_file', 'c.json']).infer_ema is None
