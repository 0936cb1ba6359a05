"""`--ema_decay` on the GPU: the shadow kept inside the optimiser launch (comic_adam_tf_ema / comic_momentum_tf_ema) against
tests/ema_ref.py on the device's own variables, behind the ranges, the voided-step gate and the clip; the trajectory through
training steps; `model_ema-N`, `--infer_ema` and `--infer_average` through the CLIs."""
import glob
import importlib.util
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import comic_amd._lib as L
from comic_amd import checkpoint as ckpt, decoder as cdec, optim
from tests import ema_ref
from tests.ema_ref import EMA_TOL
from tests.gpu_util import DEV, assert_close, dev, lib, rel_err, stream, sync

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64            # sentinel floats behind the n elements: a launch may not write past its range
OMD = 0.1


def _padded(a):
    return dev(np.concatenate([a, np.full(PAD, 7.5, np.float32)]))


def _tail_untouched(*bufs):
    return all(bool((b[-PAD:] == 7.5).all()) for b in bufs)


# ---- 1. op level, Adam ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [100003, 1, 255, 256, 257])
def test_adam_ema_entry(n):
    """The EMA launch writes the w, m, v of comic_adam_tf_gated bit for bit; the shadow is s + (w_out - s) * omd on the
    device's own w_out (float64 reference, 1e-6); nothing past n is written; a set status word leaves all five buffers."""
    rng = np.random.default_rng(n)
    w, g, s = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    m = (0.1 * rng.standard_normal(n)).astype(np.float32)
    v = (0.1 * rng.random(n)).astype(np.float32)
    t, lr, l2 = 3, 1e-2, 1e-5
    lr_t = lr * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
    dg = dev(g)
    a, b, ds = [_padded(x) for x in (w, m, v)], [_padded(x) for x in (w, m, v)], _padded(s)
    L.check(lib().comic_adam_tf_gated(a[0].data_ptr(), dg.data_ptr(), a[1].data_ptr(), a[2].data_ptr(), n, lr_t, 0.9, 0.999,
                                      1e-2, l2, 0.5, None, stream()))
    L.check(lib().comic_adam_tf_ema(b[0].data_ptr(), dg.data_ptr(), b[1].data_ptr(), b[2].data_ptr(), n, lr_t, 0.9, 0.999,
                                    1e-2, l2, 0.5, None, ds.data_ptr(), OMD, stream()))
    sync()
    for x, y, name in zip(a, b, 'wmv'):
        assert torch.equal(x, y), name
    assert not torch.equal(b[0][:n], dev(w)) and _tail_untouched(ds, *b)
    want = ema_ref.update(s, b[0][:n].cpu().numpy(), OMD)
    e = rel_err(ds[:n].cpu().numpy(), want)
    print('adam ema n=%d: shadow rel err %.3e' % (n, e))
    assert_close(ds[:n].cpu().numpy(), want, EMA_TOL, 'adam shadow')
    # a voided step: w, m, v and the shadow stay
    flag = dev(np.ones(1, np.float32))
    before = [x.clone() for x in b + [ds]]
    L.check(lib().comic_adam_tf_ema(b[0].data_ptr(), dg.data_ptr(), b[1].data_ptr(), b[2].data_ptr(), n, lr_t, 0.9, 0.999,
                                    1e-2, l2, 0.5, flag.data_ptr(), ds.data_ptr(), OMD, stream()))
    sync()
    assert all(torch.equal(x, y) for x, y in zip(before, b + [ds]))


def test_ema_entries_refuse_bad_arguments():
    x = [dev(np.zeros(8, np.float32)) for _ in range(5)]
    p = [t.data_ptr() for t in x]
    for shadow, omd, n in ((None, 0.1, 8), (p[4], 0.0, 8), (p[4], 1.5, 8), (p[4], float('nan'), 8), (p[4], 0.1, 0)):
        with pytest.raises(L.ComicHipError):
            L.check(lib().comic_adam_tf_ema(p[0], p[1], p[2], p[3], n, 1e-2, 0.9, 0.999, 1e-2, 0.0, 1.0, None, shadow, omd,
                                            stream()))
        with pytest.raises(L.ComicHipError):
            L.check(lib().comic_momentum_tf_ema(p[0], p[1], p[2], n, 1e-2, 0.9, 0.0, 1.0, None, shadow, omd, stream()))
    sync()
    assert all(float(t.abs().max()) == 0.0 for t in x)
    L.check(lib().comic_adam_tf_ema(p[0], p[1], p[2], p[3], 8, 1e-2, 0.9, 0.999, 1e-2, 0.0, 1.0, None, p[4], 1.0, stream()))
    sync()


# ---- 2. op level, Momentum -----------------------------------------------------------------------------------------------
def test_momentum_ema_entry():
    rng = np.random.default_rng(8)
    n = 70001
    w, s = (rng.standard_normal(n).astype(np.float32) for _ in range(2))
    a, b, ds = [_padded(x) for x in (w, np.zeros(n, np.float32))], [_padded(x) for x in (w, np.zeros(n, np.float32))], _padded(s)
    lr, l2 = 1e-2, 1e-5
    for it in range(2):
        dg = dev(rng.standard_normal(n).astype(np.float32))
        s_in = ds[:n].cpu().numpy()
        L.check(lib().comic_momentum_tf_gated(a[0].data_ptr(), dg.data_ptr(), a[1].data_ptr(), n, lr, 0.9, l2, 0.5, None,
                                              stream()))
        L.check(lib().comic_momentum_tf_ema(b[0].data_ptr(), dg.data_ptr(), b[1].data_ptr(), n, lr, 0.9, l2, 0.5, None,
                                            ds.data_ptr(), OMD, stream()))
        sync()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), it
        want = ema_ref.update(s_in, b[0][:n].cpu().numpy(), OMD)
        print('momentum ema update %d: shadow rel err %.3e' % (it, rel_err(ds[:n].cpu().numpy(), want)))
        assert_close(ds[:n].cpu().numpy(), want, EMA_TOL, 'momentum shadow')
    assert _tail_untouched(ds, *b)
    flag = dev(np.ones(1, np.float32))
    before = [x.clone() for x in b + [ds]]
    L.check(lib().comic_momentum_tf_ema(b[0].data_ptr(), dg.data_ptr(), b[1].data_ptr(), n, lr, 0.9, l2, 0.5, flag.data_ptr(),
                                        ds.data_ptr(), OMD, stream()))
    sync()
    assert all(torch.equal(x, y) for x, y in zip(before, b + [ds]))


# ---- 3. ranges and gate --------------------------------------------------------------------------------------------------
def _seeded_buffers(spec):
    g = torch.Generator(device='cpu').manual_seed(3)
    PP = cdec.FlatParams(spec.param_shapes(), DEV, status_tail=True)
    GG = cdec.FlatParams(spec.param_shapes(), DEV, status_tail=True)
    PP.data[:PP.numel].copy_(torch.randn(PP.numel, generator=g))
    GG.data[:GG.numel].copy_(torch.randn(GG.numel, generator=g))
    return PP, GG


@pytest.mark.parametrize('opt_name', ['adam', 'sgd'])
def test_ema_update_by_ranges_equals_one_launch(opt_name):
    """test_optimiser_update_by_ranges_equals_one_launch with a shadow: the four ranges in reverse give the bits of the
    one-launch step in w, the slots AND the shadow; the shadow-less optimiser gives the same w and slots; a voided step
    leaves the shadow of step 1 in every range."""
    from comic_amd.trainer import DataParallel
    spec = cdec.DecoderSpec(M=25, C=2048, Cg=2048)
    outs = []
    for mode in ('flat', 'ranges', 'ranges_void', 'no_ema'):
        PP, GG = _seeded_buffers(spec)
        opt = optim.make_optimiser(opt_name, PP, ema_decay=0.0 if mode == 'no_ema' else 0.9)
        if mode == 'no_ema':
            assert opt.ema is None
        else:
            assert torch.equal(opt.ema.flat, PP.flat)           # starts at the variables
        seen = []
        for step in range(2):
            if mode in ('flat', 'no_ema'):
                opt.step(GG, 1e-2, grad_scale=0.5)
            else:
                if mode == 'ranges_void' and step == 1:
                    GG.data[GG.numel] = 1.0
                rng_ = DataParallel.chunk_bounds(GG, 4)[::-1]
                opt.step(GG, 1e-2, grad_scale=0.5, ranges=rng_, before_range=seen.append)
            if step == 0 and mode == 'flat':
                sync()
                first = (PP.data.clone(), opt.ema.data.clone())
        sync()
        assert mode in ('flat', 'no_ema') or seen == [0, 1, 2, 3] * 2
        outs.append((PP.data.clone(), opt.m.data.clone(), opt.v.data.clone(),
                     opt.ema.data.clone() if opt.ema is not None else None, opt.t))
    flat, ranges, void, plain = outs
    assert all(torch.equal(a, b) for a, b in zip(flat[:4], ranges[:4])) and flat[4] == ranges[4] == 2
    assert all(torch.equal(a, b) for a, b in zip(flat[:3], plain[:3]))
    assert not torch.equal(flat[3][:PP.numel], flat[0][:PP.numel])          # a shadow, not a copy
    assert torch.equal(void[0][:PP.numel], first[0][:PP.numel]) and torch.equal(void[3], first[1])
    assert not torch.equal(void[3], flat[3])
    # the two updates' shadow: warm-up rates 1/10 and 2/11 on the device's own variables
    want = ema_ref.replay(_seeded_buffers(spec)[0].flat.cpu().numpy(),
                          [first[0][:PP.numel].cpu().numpy(), flat[0][:PP.numel].cpu().numpy()], 0.9)
    assert_close(flat[3][:PP.numel].cpu().numpy(), want, EMA_TOL, 'shadow after two updates')


# ---- 4. clip + EMA -------------------------------------------------------------------------------------------------------
def test_clip_and_ema():
    """The setting of test_gradient_clipping_matches_oracle: the clip rewrites g in front of the update and does not see
    the shadow; the parameters are those of the step without a shadow, bit for bit."""
    rng = np.random.default_rng(11)
    shapes = {'a': (3, 5000), 'b': (700,), 'c': (), 'd': (40000,), 'e': (128, 64)}
    scale_of = {'a': 1.0, 'b': 1e-3, 'c': 50.0, 'd': 0.2, 'e': 1e-2}
    w = {k: rng.standard_normal(shapes[k]).astype(np.float32) for k in shapes}
    g = {k: (scale_of[k] * rng.standard_normal(shapes[k])).astype(np.float32) for k in shapes}
    clip, l2, gs, lr = 2.5, 1e-3, 0.5, 1e-2
    res = {}
    for decay in (0.0, 0.9):
        PP = cdec.FlatParams(shapes, DEV, status_tail=True)
        G = PP.like()
        PP.load(w); G.load(g)
        opt = optim.AdamTF(PP, l2_decay=l2, clip_norm=clip, ema_decay=decay)
        opt.step(G, lr, grad_scale=gs)
        sync()
        res[decay] = (PP, G, opt)
    (P0, G0, _), (P1, G1, opt) = res[0.0], res[0.9]
    assert torch.equal(P0.data, P1.data) and torch.equal(G0.data, G1.data)
    got, new = opt.ema.to_numpy(), P1.to_numpy()
    for k in shapes:
        assert_close(got[k], ema_ref.update(w[k], new[k], 1.0 - ema_ref.rate(0.9, 1)), EMA_TOL, 'clipped shadow ' + k)
    # the voided step touches nothing
    G1.status.fill_(1.0)
    before = (P1.data.clone(), G1.data.clone(), opt.ema.data.clone(), opt.m.data.clone(), opt.v.data.clone())
    opt.step(G1, lr, grad_scale=gs)
    sync()
    assert all(torch.equal(x, y) for x, y in zip(before, (P1.data, G1.data, opt.ema.data, opt.m.data, opt.v.data)))


# ---- 5. trajectory through the training step -----------------------------------------------------------------------------
def test_ema_trajectory_through_training_steps():
    """12 decoder training steps with ema_decay 0.5 (updates 1-8 on the warm-up rate, from update 9 = n 8 on the fixed one):
    the final shadow equals the float64 replay of the recurrence on the parameters the device held after every step, per
    variable at 1e-6; the parameters after every step are those of the run without a shadow, bit for bit."""
    spec = cdec.DecoderSpec(D=128, E=64, M=25, C=2048, Cg=2048)
    p = cdec.init_params(spec, 0)
    rng = np.random.default_rng(5)
    B, T = 4, 6
    fm = dev(rng.standard_normal((B, spec.M, spec.C)).astype(np.float32))
    im = dev(rng.standard_normal((B, spec.Cg)).astype(np.float32))
    caps = np.full((B, T), -1, np.int64)
    for b in range(B):
        n = T - 2 if b == 0 else int(rng.integers(1, T - 1))
        caps[b, 0], caps[b, 1:1 + n], caps[b, 1 + n] = spec.start_id, rng.integers(0, 256, n), spec.end_id
    runs = {}
    for decay in (0.5, 0.0):
        dec = cdec.Decoder(spec, p, DEV, seed=3)
        opt = optim.AdamTF(dec.params, ema_decay=decay)
        w0, traj = dec.params.flat.cpu().numpy().copy(), []
        for it in range(12):
            dec.train_step(fm, im, caps, training=True, seed=70 + it)
            opt.step(dec.grads, 1e-2)
            sync()
            traj.append(dec.params.flat.cpu().numpy().copy())
        runs[decay] = (w0, traj, opt, dec)
    w0, traj, opt, dec = runs[0.5]
    assert dec.voided_steps() == 0 and not np.array_equal(traj[-1], traj[-2])
    for a, b in zip(traj, runs[0.0][1]):
        np.testing.assert_array_equal(a, b)
    assert np.array_equal(w0, runs[0.0][0]) and runs[0.0][2].ema is None
    want, got = ema_ref.replay(w0, traj, 0.5), opt.ema.flat.cpu().numpy()
    worst = 0.0
    for k, shp in spec.param_shapes().items():
        lo = dec.params.offsets[k]
        hi = lo + (int(np.prod(shp)) if len(shp) else 1)
        worst = max(worst, rel_err(got[lo:hi], want[lo:hi]))
        assert_close(got[lo:hi], want[lo:hi], EMA_TOL, 'shadow of ' + k)
    print('trajectory: worst per-variable shadow rel err %.3e' % worst)
    assert rel_err(got, traj[-1]) > 1e-4                    # the shadow lags the variables


# ---- 6. / 7. the CLIs ----------------------------------------------------------------------------------------------------
def _run(name, argv):
    spec = importlib.util.spec_from_file_location('cli_%s_gpu_ema' % name, os.path.join(ROOT, 'src', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(argv)


def _no_error_files(logs):
    errs = glob.glob(os.path.join(logs, 'mscoco', 'error__*'))
    assert not errs, open(errs[0]).read()


def _step_of(path):
    return int(os.path.basename(path).split('-')[-1].split('.')[0])


RUN_NAME = 'radix_b256_add_LN_softmax_h8_tie_lstm_run_01'
MEM_KERNEL = 'Model/decoder/rnn_decoder/memory_layer/kernel'


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """The tiny dataset and decoder-mode flags of test_train_infer_scst_cli, trained twice: plain, and with --ema_decay 0.9."""
    from tests import tiny_dataset
    root = tmp_path_factory.mktemp('ema_cli')
    ds = tiny_dataset.make(str(root / 'mscoco'), n_train=16, n_valid=4, n_test=4)
    out = dict(ds=ds, root=root)
    for tag, more in (('plain', []), ('ema', ['--ema_decay', '0.9'])):
        logs = str(root / ('experiments_' + tag))
        common = ['--dataset_dir', ds, '--log_root', logs, '--cnn_name', 'inception_v3', '--cnn_fm_attention', 'Mixed_7c',
                  '--cnn_input_size', '139,139', '--batch_size_eval', '4', '--rnn_size', '128', '--rnn_word_size', '64']
        _run('train', common + ['--train_mode', 'decoder', '--batch_size_train', '8', '--max_epoch', '2'] + more)
        _no_error_files(logs)
        out[tag] = dict(logs=logs, common=common, run_dir=os.path.join(logs, 'mscoco', RUN_NAME))
    return out


def _infer(run_dir, ds, more=()):
    _run('infer', ['--infer_checkpoints_dir', run_dir, '--dataset_dir', ds, '--infer_set', 'test', '--batch_size_infer', '2',
                   '--get_metric_score', ''] + list(more))


def test_cli_decoder_mode_writes_and_reads_the_averaged_weights(runs):
    from comic_amd import configuration as conf, model as mdl, train_fn as train
    ds, plain, ema = runs['ds'], runs['plain']['run_dir'], runs['ema']['run_dir']
    compact = sorted(glob.glob(os.path.join(ema, 'model_compact-*.npz')), key=_step_of)
    assert compact and [os.path.basename(f) for f in compact] == \
        [os.path.basename(f) for f in sorted(glob.glob(os.path.join(plain, 'model_compact-*.npz')), key=_step_of)]
    # the shadow changes nothing in what is trained: every compact checkpoint of the two runs holds the same arrays
    for f in compact:
        a, b = np.load(f), np.load(os.path.join(plain, os.path.basename(f)))
        assert set(a.files) == set(b.files)
        for k in a.files:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert not glob.glob(os.path.join(plain, 'model_ema-*'))
    assert not hasattr(conf.load_config(os.path.join(plain, 'config.pkl')), 'ema_decay')
    assert conf.load_config(os.path.join(ema, 'config.pkl')).ema_decay == 0.9
    # model_ema-N: the compact checkpoint's names, the shadow in place of the trained variables, the CNN copied
    for f in compact:
        a, e = np.load(f), np.load(f.replace('model_compact-', 'model_ema-'))
        assert set(a.files) == set(e.files)
        assert a[MEM_KERNEL].shape == e[MEM_KERNEL].shape and not np.array_equal(a[MEM_KERNEL], e[MEM_KERNEL])
        assert int(a['global_step']) == int(e['global_step'])
        for k in a.files:
            if k.startswith(ckpt.CNN_SCOPE):
                np.testing.assert_array_equal(a[k], e[k], err_msg=k)
    # model-N carries the shadow with the slots; a resumed model loads it, any other model starts it at its variables
    full = sorted(glob.glob(os.path.join(ema, 'model-*.npz')), key=_step_of)[-1]
    shadow = np.load(full)['optimise/caption/ema']
    last = np.load(compact[-1].replace('model_compact-', 'model_ema-'))
    for resume in (True, False):
        c = conf.load_config(os.path.join(ema, 'config.pkl'))
        c.resume_training, c.checkpoint_path = resume, ema
        mdl.reset_default_graph()
        man = train._manager(c)
        try:
            m = mdl.CaptionModel(c, mode='train', batch_ops=man.batch_train, reuse=False, name='train', device=DEV)
            m.restore_model()
            sync()
            assert shadow.shape == (m.decoder.params.numel,) and shadow.dtype == np.float32
            if resume:
                assert np.array_equal(m.opt.ema.flat.cpu().numpy(), shadow) and m.global_step == _step_of(full)
                assert not torch.equal(m.opt.ema.flat, m.decoder.params.flat)
                names = ckpt.decoder_var_names(m.spec)
                by_name = {names[k]: v for k, v in m.opt.ema.to_numpy().items()}
                assert np.array_equal(by_name[MEM_KERNEL], last[MEM_KERNEL])        # what model_ema-N holds
            else:
                assert torch.equal(m.opt.ema.flat, m.decoder.params.flat) and m.global_step == 0
        finally:
            man.close()
            mdl.reset_default_graph()
    # --infer_ema decodes model_ema-N into a directory of its own: the captions of plain infer.py on that file
    n = str(_step_of(compact[-1]))
    _infer(ema, ds, ['--infer_ema', '--infer_checkpoints', n])
    got = json.load(open(os.path.join(ema, 'infer_test_beam_3_lpen_0.0_ema', 'captions___%s.json' % n)))
    assert len(got) == 4 and all(set(d) == {'image_id', 'caption'} for d in got)
    assert not os.path.exists(os.path.join(ema, 'infer_test_beam_3_lpen_0.0'))
    alone = str(runs['root'] / 'ema_as_compact')
    os.makedirs(alone)
    shutil.copy(os.path.join(ema, 'config.pkl'), alone)
    shutil.copy(os.path.join(ema, 'model_ema-%s.npz' % n), os.path.join(alone, 'model_compact-%s.npz' % n))
    _infer(alone, ds)
    assert got == json.load(open(os.path.join(alone, 'infer_test_beam_3_lpen_0.0', 'captions___%s.json' % n)))
    # a run without --ema_decay has nothing to decode
    with pytest.raises(ValueError, match='--ema_decay'):
        _infer(plain, ds, ['--infer_ema'])
    # --infer_average: the mean of two checkpoints as one model.  Two epochs of this size save once (the reference's cadence
    # keeps the last 100 steps for the final save), so the run is resumed for a third epoch: the second checkpoint, and
    # the shadow of a run resumed through the CLI goes on from the saved one
    _run('train', runs['ema']['common'] + ['--train_mode', 'decoder', '--batch_size_train', '8', '--max_epoch', '3'])
    _no_error_files(runs['ema']['logs'])
    compact = sorted(glob.glob(os.path.join(ema, 'model_compact-*.npz')), key=_step_of)
    nums = [str(_step_of(f)) for f in compact]
    assert len(nums) == 2 and os.path.isfile(os.path.join(ema, 'model_ema-%s.npz' % nums[-1]))
    resumed = np.load(sorted(glob.glob(os.path.join(ema, 'model-*.npz')), key=_step_of)[-1])
    assert int(resumed['global_step']) == int(nums[-1]) and not np.array_equal(resumed['optimise/caption/ema'], shadow)
    a, b = nums[0], nums[-1]
    _infer(ema, ds, ['--infer_average', '--infer_checkpoints', '%s,%s' % (a, b)])
    avg_dir = os.path.join(ema, 'infer_test_beam_3_lpen_0.0_avg_%s+%s' % (a, b))
    caps = glob.glob(os.path.join(avg_dir, 'captions___*.json'))
    assert len(caps) == 1 and len(json.load(open(caps[0]))) == 4
    mean = np.load(os.path.join(avg_dir, 'model_compact-%s.npz' % b))
    za, zb = np.load(compact[0]), np.load(compact[-1])
    assert np.array_equal(mean[MEM_KERNEL], ((za[MEM_KERNEL].astype(np.float64) + zb[MEM_KERNEL]) / 2).astype(np.float32))


def test_cli_cnn_finetune_tf_bundle_carries_the_cnn_shadows(runs):
    """cnn_finetune --checkpoint_format tf --ema_decay 0.9 on top of the EMA decoder run."""
    from comic_amd import tf_bundle
    e = runs['ema']
    _run('train', e['common'] + ['--train_mode', 'cnn_finetune', '--batch_size_train', '8', '--max_epoch', '1',
                                 '--checkpoint_format', 'tf', '--ema_decay', '0.9'])
    _no_error_files(e['logs'])
    ft_dir = e['run_dir'].replace('_run_01', '_cnnFT_run_01')
    idx = sorted(glob.glob(os.path.join(ft_dir, 'model_ema-*.index')), key=_step_of)
    assert idx, os.listdir(ft_dir)
    shadow = tf_bundle.read_bundle(idx[-1][:-len('.index')])
    compact = tf_bundle.read_bundle(idx[-1][:-len('.index')].replace('model_ema-', 'model_compact-'))
    stage0 = np.load(sorted(glob.glob(os.path.join(e['run_dir'], 'model_compact-*.npz')), key=_step_of)[-1])
    assert set(shadow) == set(compact)
    base = 'Model/encoder/cnn/InceptionV3/Mixed_7c/Branch_0/Conv2d_0a_1x1/'
    k, kb, km = base + 'weights', base + 'BatchNorm/beta', base + 'BatchNorm/moving_mean'
    assert shadow[k].shape == compact[k].shape == stage0[k].shape
    assert not np.array_equal(shadow[k], compact[k]) and not np.array_equal(shadow[k], stage0[k])
    np.testing.assert_array_equal(shadow[km], compact[km])          # BN statistics: frozen, no shadow
    np.testing.assert_array_equal(shadow[km], stage0[km])
    assert not np.array_equal(shadow[MEM_KERNEL], compact[MEM_KERNEL])
    full = tf_bundle.read_bundle(sorted(glob.glob(os.path.join(ft_dir, 'model-*.index')), key=_step_of)[-1][:-len('.index')])
    sfx = '/ExponentialMovingAverage'
    assert full[k + sfx].shape == compact[k].shape and full[kb + sfx].shape == compact[kb].shape
    np.testing.assert_array_equal(full[k + sfx], shadow[k])
    np.testing.assert_array_equal(full[kb + sfx], shadow[kb])
    np.testing.assert_array_equal(full[MEM_KERNEL + sfx], shadow[MEM_KERNEL])
    assert not any(n.endswith('moving_mean' + sfx) or n.endswith('moving_variance' + sfx) for n in full)
    assert not any('cnn_w_ema' in n or n == 'optimise/caption/ema' for n in full)


def test_cli_legacy_head_shadows_in_both_files_and_resume(tmp_path):
    """--legacy (the LN_tanh + im_embed head is trained) with --checkpoint_format tf --ema_decay 0.9: the head's shadows under
    `<variable>/ExponentialMovingAverage` in model-N, their values as the head's variables in model_ema-N, and a second
    invocation resumes from the bundle with the shadows loaded (not reset to the variables)."""
    from tests import tiny_dataset
    from comic_amd import tf_bundle
    from comic_amd.encoder_head import TF_NAMES
    ds = tiny_dataset.make(str(tmp_path / 'mscoco'), n_train=8, n_valid=4, n_test=4)
    logs = str(tmp_path / 'experiments')
    args = ['--dataset_dir', ds, '--log_root', logs, '--batch_size_eval', '4', '--rnn_size', '128', '--rnn_word_size', '64',
            '--train_mode', 'decoder', '--batch_size_train', '4', '--legacy', 'True', '--checkpoint_format', 'tf',
            '--ema_decay', '0.9']
    _run('train', args + ['--max_epoch', '1'])
    _no_error_files(logs)
    run_dir, = glob.glob(os.path.join(logs, 'mscoco', '*_run_01'))

    def newest(prefix):
        return tf_bundle.read_bundle(sorted(glob.glob(os.path.join(run_dir, prefix + '-*.index')), key=_step_of)[-1][:-len('.index')])
    full, shadow, compact = newest('model'), newest('model_ema'), newest('model_compact')
    assert set(shadow) == set(compact)
    sfx = '/ExponentialMovingAverage'
    for v in list(TF_NAMES.values()) + [MEM_KERNEL]:
        np.testing.assert_array_equal(full[v + sfx], shadow[v], err_msg=v)
        np.testing.assert_array_equal(full[v], compact[v], err_msg=v)
        assert not np.array_equal(shadow[v], compact[v]), v
    assert not any('head_ema' in n or n == 'optimise/caption/ema' for n in full)
    step1 = int(full['global_step'])
    _run('train', args + ['--max_epoch', '2'])          # the run directory exists: resumes
    _no_error_files(logs)
    full2, shadow2 = newest('model'), newest('model_ema')
    assert int(full2['global_step']) == 2 * step1
    # a shadow that had been reset to the variables at the resume would have forgotten the first epoch: with the fixed decay
    # 0.9 from update 10 on, the first epoch's shadow still weighs 0.9^step1 in the second epoch's
    w = TF_NAMES['W']
    np.testing.assert_array_equal(full2[w + sfx], shadow2[w])
    assert not np.array_equal(shadow2[w], shadow[w]) and not np.array_equal(shadow2[w], full2[w])
