"""Soft-target XE training on the GPU: the soft loss launch (comic_xent_soft) and the teacher's table
(comic_teacher_topk) on their own operands against float64 numpy (tests/soft_targets_ref.py), and the whole step through
Decoder.train_step(soft=, teacher=) against the float64 oracle.  The operands come from the shared builders of
tests/soft_targets_ref.py; tests/test_soft_targets_cpu.py holds the input condition of the exact-id comparisons.  Outputs
are NaN (ids -1) before a launch; each figure is printed before it is asserted (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from comic_amd import decoder as cdec
from oracle import decoder_ref as dr
from tests import soft_targets_ref as S
from tests.exec_ops_ref import XENT_TOL
from tests.gpu_util import DEV, F32_RTOL, assert_close, dev, elementwise_excess, lib, rel_err, stream, sync

NAN = float('nan')


def nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def chk(name, got, ref, tol, elementwise=None):
    got, ref = np.asarray(got), np.asarray(ref, np.float64)
    print('  %-40s err %.3e  element-wise %.3e  bar %.1e' % (name, rel_err(got, ref), elementwise_excess(got, ref, 1.0), tol))
    return assert_close(got, ref, tol, name, elementwise=elementwise)


# ================================================================================ the soft loss launch ===============
def launch_xent_soft(c, V, ld_dl, eps, lam, K, table=True, entry='comic_xent_soft'):
    d_logits = dev(c['logits'])
    rows = S.T_ROWS * S.B
    loss, nll, dl = nan(rows), nan(rows), nan(rows * ld_dl)
    ids = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    keep = [dev(c[k]) for k in ('targets', 'coef', 'wmask', 'lens')] + [dev(c['t_ids']), dev(c['t_probs'])]
    tg, cf, wm, ln, ti, tp = (t.data_ptr() for t in keep)
    if entry == 'comic_op_xent':
        assert ld_dl == V
        rc = lib().comic_op_xent(d_logits.data_ptr(), tg, cf, wm, ln, loss.data_ptr(), dl.data_ptr(), ids.data_ptr(), S.T_ROWS,
                                 S.T_STRIDE, S.B, V, stream())
    else:
        rc = lib().comic_xent_soft(d_logits.data_ptr(), tg, cf, wm, ln, loss.data_ptr(), nll.data_ptr(), dl.data_ptr(), ld_dl,
                                   ids.data_ptr(), S.T_ROWS, S.T_STRIDE, S.B, V, eps, lam, K, ti if table else None,
                                   tp if table else None, stream())
    sync()
    assert rc == 0, lib().comic_last_error()
    return d_logits, loss, nll, dl, ids


@pytest.mark.parametrize('regime', [None, 'peaked'], ids=['normal', 'peaked'])
@pytest.mark.parametrize('eps,lam', S.SETTINGS)
@pytest.mark.parametrize('K', S.K_CASES)
@pytest.mark.parametrize('V,pad', [(258, 0), (258, 2), (4099, 0), (4099, 1)])
def test_xent_soft_matches_reference(V, pad, K, eps, lam, regime):
    """loss rows and nll rows at XENT_TOL element-wise, d logits at F32_RTOL, ids exact, the finished row zeroed in place
    and the padding columns of d logits exactly zero; targets inside and outside the teacher's ids"""
    c = S.xent_case(V, K, regime)
    ld_dl = V + pad
    d_logits, loss, nll, dl, ids = launch_xent_soft(c, V, ld_dl, eps, lam, K, table=lam > 0)
    ref = S.soft_xent_ref(c['logits'], c['targets'], c['coef'], c['wmask'], c['lens'], eps, lam, c['t_ids'][:S.T_ROWS],
                          c['t_probs'][:S.T_ROWS])
    np.testing.assert_array_equal(host(d_logits), ref['logits'])
    chk('loss rows', host(loss).reshape(S.T_ROWS, S.B), ref['loss'], XENT_TOL, True)
    chk('nll rows', host(nll).reshape(S.T_ROWS, S.B), ref['nll'], XENT_TOL, True)
    d = host(dl).reshape(S.T_ROWS, S.B, ld_dl)
    chk('dlogits', d[..., :V], ref['dlogits'], F32_RTOL)
    assert (d[..., V:] == 0).all(), 'padding columns of d logits are not exactly zero'
    np.testing.assert_array_equal(host(ids).reshape(S.T_ROWS, S.B), ref['ids'])
    assert ref['loss'][2, 1] == 0 and ref['loss'][1, 2] == 0 and (ref['loss'] > 0).sum() == 7     # a finished row, a weightless token


@pytest.mark.parametrize('regime', [None, 'peaked'], ids=['normal', 'peaked'])
@pytest.mark.parametrize('V', S.V_CASES)
def test_xent_soft_without_soft_targets_is_the_hard_loss(V, regime):
    """eps = lam = 0: the soft entry agrees with comic_op_xent within XENT_TOL, and its nll rows are its loss rows"""
    c = S.xent_case(V, 1, regime)
    _, loss_h, _, dl_h, ids_h = launch_xent_soft(c, V, V, 0.0, 0.0, 0, entry='comic_op_xent')
    _, loss_s, nll_s, dl_s, ids_s = launch_xent_soft(c, V, V, 0.0, 0.0, 0, table=False)
    chk('loss rows', host(loss_s), host(loss_h), XENT_TOL, True)
    chk('dlogits', host(dl_s), host(dl_h), XENT_TOL)
    assert torch.equal(loss_s, nll_s) and torch.equal(ids_s, ids_h)


def test_xent_soft_refusals():
    c = S.xent_case(258, 8)
    t = {k: dev(v) for k, v in c.items()}
    out = nan(S.T_ROWS * S.B * 258)

    def call(eps, lam, K, table=True):
        return lib().comic_xent_soft(t['logits'].data_ptr(), t['targets'].data_ptr(), t['coef'].data_ptr(), t['wmask'].data_ptr(),
                                     t['lens'].data_ptr(), None, None, out.data_ptr(), 258, None, S.T_ROWS, S.T_STRIDE, S.B, 258,
                                     eps, lam, K, t['t_ids'].data_ptr() if table else None,
                                     t['t_probs'].data_ptr() if table else None, stream())
    for args, word in (((-0.1, 0.0, 8), b'smoothing'), ((1.0, 0.0, 8), b'smoothing'), ((0.0, 1.5, 8), b'teacher_weight'),
                       ((0.6, 0.5, 8), b'exceeds 1'), ((0.0, 0.5, 0), b'K 0'), ((0.0, 0.5, 33), b'K 33'),
                       ((0.0, 0.5, 8, False), b'without a teacher table')):
        assert call(*args) == 2 and word in lib().comic_last_error(), (args, lib().comic_last_error())
    sync()
    assert bool(torch.isnan(out).all())                                     # refused before any launch


# ================================================================================ the teacher's table ================
def launch_topk(z, weights, lens, Tp, V, tau, K):
    T, B = z[0].shape[:2]
    zd = [dev(x) for x in z]
    ids = torch.full((T, B, K), -1, dtype=torch.int32, device=DEV)
    probs = nan(T, B, K)
    ptrs = (C.c_void_p * len(z))(*[x.data_ptr() for x in zd])
    w = (C.c_float * len(z))(*weights)
    d_lens = dev(np.asarray(lens, np.int32))
    rc = lib().comic_teacher_topk(ptrs, w, len(z), d_lens.data_ptr(), B, T, Tp, V, tau, K, ids.data_ptr(), probs.data_ptr(),
                                  stream())
    sync()
    assert rc == 0, lib().comic_last_error()
    return ids, probs


@pytest.mark.parametrize('V,K,n,tau', S.TEACHER_CASES)
def test_teacher_topk_matches_reference(V, K, n, tau):
    """ids exact (the rank gaps of these operands exceed 1e-5: tests/test_soft_targets_cpu.py), probs within 1e-5 relative
    element by element, rows without a token as ids 0 .. K-1 / probs 0, and the same bits from a second run"""
    z = S.teacher_logits(V, n)
    Tp = S.T_ROWS
    ids, probs = launch_topk(z, S.WEIGHTS[n], S.LENS, Tp, V, tau, K)
    r_ids, r_probs, _ = S.teacher_topk_ref(z, S.WEIGHTS[n], S.LENS, Tp, tau, K)
    np.testing.assert_array_equal(host(ids), r_ids)
    live = r_probs[..., 0] > 0
    assert live.sum() == 8 and (~live).sum() == 4                           # t = 3 is past T', (t = 2, b = 1) past lens
    rel = np.abs(host(probs).astype(np.float64) - r_probs)[live] / r_probs[live]
    print('  probs: largest relative error %.3e  bar 1.0e-05' % rel.max())
    assert rel.max() <= 1e-5
    assert (host(probs)[~live] == 0).all()
    ids2, probs2 = launch_topk(z, S.WEIGHTS[n], S.LENS, Tp, V, tau, K)
    assert torch.equal(ids, ids2) and torch.equal(probs, probs2)


@pytest.mark.parametrize('V', S.V_CASES)
def test_teacher_topk_exact_ties_go_to_the_lowest_id(V):
    """row (0, 0): every logit equal -> ids 0 .. K-1; row (0, 1): columns 5 and V-2 share the largest logit and columns 3
    and V-1 the next, K = 3 -> 5, V-2, then 3 (the tie at the boundary goes to the lower id)"""
    K = 3
    z = S.teacher_logits(V, 3)
    for m in z:
        m[0, 0] = 0.25
        m[0, 1, [5, V - 2]] = 30.0
        m[0, 1, [3, V - 1]] = 20.0
    ids, probs = launch_topk(z, S.WEIGHTS[3], S.LENS, S.T_ROWS, V, 2.0, K)
    assert host(ids)[0, 0].tolist() == [0, 1, 2] and host(ids)[0, 1].tolist() == [5, V - 2, 3]
    p = host(probs)
    assert p[0, 0, 0] == p[0, 0, 2] and p[0, 1, 0] == p[0, 1, 1]
    r_ids, _, _ = S.teacher_topk_ref(z, S.WEIGHTS[3], S.LENS, S.T_ROWS, 2.0, K)
    np.testing.assert_array_equal(host(ids)[0, :2], r_ids[0, :2])


def test_teacher_topk_refusals():
    z = S.teacher_logits(258, 1)
    zd = dev(z[0])
    ptrs, w = (C.c_void_p * 1)(zd.data_ptr()), (C.c_float * 1)(1.0)
    lens = dev(S.LENS)
    ids = torch.full((4, 3, 32), -1, dtype=torch.int32, device=DEV)
    probs = nan(4, 3, 32)

    def call(V=258, tau=1.0, K=8, n=1, wt=w):
        return lib().comic_teacher_topk(ptrs, wt, n, lens.data_ptr(), 3, 4, 3, V, tau, K, ids.data_ptr(), probs.data_ptr(),
                                        stream())
    for kw, word in ((dict(K=0), b'K 0'), (dict(K=33), b'K 33'), (dict(tau=0.0), b'temperature'), (dict(n=9), b'members'),
                     (dict(V=40449), b'does not fit'), (dict(wt=(C.c_float * 1)(0.5)), b'sum to')):
        assert call(**kw) == 2 and word in lib().comic_last_error(), (kw, lib().comic_last_error())
    sync()
    assert bool(torch.isnan(probs).all())


# ================================================================================ the whole step =====================
def _spec_and_cfg():
    """the base geometry of tests/test_gpu_path.py"""
    spec = cdec.DecoderSpec(D=128, E=64, V=258, C=192, Cg=192, H=8, M=25)
    cfg = dr.DecoderConfig(rnn_size=spec.D, rnn_word_size=spec.E, attn_num_heads=spec.H, cnn_fm_projection=spec.fm_projection,
                           attn_alignment_method=spec.method, attn_probability_fn=spec.prob,
                           attn_context_layer=spec.context_layer, rnn_init_method=spec.init_method, token_type=spec.token_type,
                           softmax_size=spec.V, fm_channels=spec.C, im_embed_size=spec.Cg, start_id=spec.start_id,
                           end_id=spec.end_id, rnn_name=spec.rnn_name, l2_decay=0.0)
    return spec, cfg


def _batch(spec, B, L, seed):
    rng = np.random.default_rng(seed)
    fm = rng.standard_normal((B, spec.M, spec.C)).astype(np.float32)
    im = rng.standard_normal((B, spec.Cg)).astype(np.float32)
    caps = np.full((B, L), -1, np.int64)
    for b in range(B):
        n = L - 2 if b == 0 else int(rng.integers(1, L - 1))
        caps[b, 0] = spec.start_id
        caps[b, 1:1 + n] = rng.integers(0, 256, n)
        caps[b, 1 + n] = spec.end_id
    return fm, im, caps


def _params(cfg, seed):
    p = dr.init_params(cfg, seed)
    rng = np.random.default_rng(seed + 100)
    for k in ('b', 'b_o', 'ln_b'):
        p[k] = (0.1 * rng.standard_normal(p[k].shape)).astype(np.float32)
    p['ln_g'] = (1 + 0.1 * rng.standard_normal(p['ln_g'].shape)).astype(np.float32)
    return p


SOFT = cdec.SoftTargets(smoothing=0.1, teacher_weight=0.5, top_k=8, temperature=2.0)


@pytest.mark.parametrize('B,group', [(6, '1'), (6, '0'), (16, '1')], ids=['default', 'no_group_gemm', 'grouped_B16'])
def test_soft_train_step_matches_oracle(B, group, monkeypatch):
    """Decoder.train_step(soft=, teacher=) with the table of a second decoder's teacher_targets: the forward is the hard
    step's (logits and map loss in bits), loss and nll follow the rule on the step's own logits, and every gradient is the
    float64 oracle's.  train_backward is affine in X = exp(log_softmax): with G(X) its gradients at X, the soft step's are
    G(p) + G(e_y + 1) - G(q + 1).  B = 16 takes the grouped launches, where the map loss leaves the loss launch."""
    monkeypatch.setenv('COMIC_GROUP_GEMM', group)
    spec, cfg = _spec_and_cfg()
    Lc = 11
    p = _params(cfg, 3)
    fm, im, caps = _batch(spec, B, Lc, 7)
    _, targets, wmask, lens = dr.process_inputs(caps, cfg.token_type)
    Tp = int(lens.max())
    masks = dr.make_dropout_masks(cfg, B, Tp, spec.M, 11)
    teacher = cdec.Decoder(spec, _params(cfg, 4), DEV)
    t_ids, t_probs = teacher.teacher_targets(dev(fm), dev(im), caps, SOFT.top_k, SOFT.temperature)
    hard_dec, dec = cdec.Decoder(spec, p, DEV), cdec.Decoder(spec, p, DEV)
    hard = hard_dec.train_step(dev(fm), dev(im), caps, masks=masks, training=True, want_input_grads=True)
    res = dec.train_step(dev(fm), dev(im), caps, masks=masks, training=True, want_input_grads=True, soft=SOFT,
                         teacher=(t_ids, t_probs))
    sync()
    assert torch.equal(res['logits'], hard['logits']) and torch.equal(res['attn_maps'], hard['attn_maps'])
    assert float(res['map_loss']) == float(hard['map_loss'])
    assert float(hard['nll']) == float(hard['loss'])
    # the table against the rule on the teacher's own logits (rows without a token: ids 0 .. K-1, probs 0)
    tctx = teacher._forward_logits(dev(fm), dev(im), caps)
    ids_h, probs_h = host(t_ids), host(t_probs)
    T = targets.shape[1]
    live = np.arange(T)[:, None] < lens[None, :]
    r_ids, r_probs, pbar = S.teacher_topk_ref([host(tctx.logits)], (1.0,), lens, Tp, SOFT.temperature, SOFT.top_k)
    with np.errstate(all='ignore'):                                         # (rows past T' of the logits buffer hold anything)
        ok = live & (S.rank_gaps(pbar, SOFT.top_k) > S.GAP_MIN)             # rows whose order float32 cannot change
    assert ok.sum() >= live.sum() - 2
    np.testing.assert_array_equal(ids_h[ok | ~live], r_ids[ok | ~live])
    assert (np.abs(probs_h - r_probs)[ok] <= 1e-5 * r_probs[ok]).all() and (probs_h[~live] == 0).all()
    # loss and nll on the step's own logits
    den = np.float64(wmask.sum()) + 1e-12
    coef = wmask / den
    logits_tb = host(res['logits']).transpose(1, 0, 2)
    ref = S.soft_xent_ref(logits_tb, targets, coef, wmask, lens, SOFT.smoothing, SOFT.teacher_weight, ids_h, probs_h)
    for name, got, want in (('loss', res['loss'], ref['loss'].sum() / den), ('nll', res['nll'], ref['nll'].sum() / den)):
        print('  %-6s %.7f  reference %.7f' % (name, float(got), want))
        assert abs(float(got) - want) <= XENT_TOL * abs(want), name
    assert float(res['nll']) != float(res['loss'])
    # gradients: the float64 oracle, three times
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    m64 = {k: v.astype(np.float64) for k, v in masks.items()}
    out = dr.train_forward(p64, cfg, fm.astype(np.float64), im.astype(np.float64), caps, m64)
    sm = np.exp(out['log_softmax'])                                            # [B,T,V]
    q = S.soft_target(targets, spec.V, SOFT.smoothing, SOFT.teacher_weight, ids_h.transpose(1, 0, 2), probs_h.transpose(1, 0, 2))
    e_y = S.soft_target(targets, spec.V, 0.0, 0.0)

    def G(X):
        o = dict(out)
        o['log_softmax'] = np.log(X)
        grads, dfm, dim = dr.train_backward(p64, cfg, o)
        return dict(grads, dfm=dfm, dim_embed=dim)
    g_p, g_e, g_q = G(sm), G(e_y + 1.0), G(q + 1.0)
    want = {k: g_p[k] + g_e[k] - g_q[k] for k in g_p}
    got = dict(dec.grads.to_numpy(), dfm=host(res['dfm']), dim_embed=host(res['dim_embed']))
    for k in want:
        assert_close(got[k], want[k], F32_RTOL, 'grad ' + k)
    assert rel_err(got['W_o'], hard_dec.grads.to_numpy()['W_o']) > 10 * F32_RTOL     # (and they are not the hard step's)


def test_soft_train_step_graph_replay_equals_eager():
    """use_graph: call 1 eager, call 2 captures, call 3 replays -- the bits of the eager step; call 4 replays with another
    table's contents (the step copies the table into its own buffers in front of the graph)"""
    spec, cfg = _spec_and_cfg()
    B, Lc = 6, 11
    p = _params(cfg, 3)
    fm, im, caps = _batch(spec, B, Lc, 7)
    teacher = cdec.Decoder(spec, _params(cfg, 4), DEV)
    a, b = cdec.Decoder(spec, p, DEV, seed=3), cdec.Decoder(spec, p, DEV, seed=3)
    for it in range(4):
        tau = 2.0 if it < 3 else 1.0
        table = tuple(t.clone() for t in teacher.teacher_targets(dev(fm), dev(im), caps, SOFT.top_k, tau))
        ra = a.train_step(dev(fm), dev(im), caps, training=True, seed=50 + it, use_graph=False, soft=SOFT, teacher=table)
        rb = b.train_step(dev(fm), dev(im), caps, training=True, seed=50 + it, use_graph=True, soft=SOFT, teacher=table)
        sync()
        assert float(ra['loss']) == float(rb['loss']) and float(ra['nll']) == float(rb['nll']), it
        assert torch.equal(a.grads.data, b.grads.data), it
        if it == 2:
            third = float(ra['loss'])
    assert [c.graph is not None for c in b._ctx.values()] == [True]
    assert float(ra['loss']) != third


def test_soft_options_the_step_refuses_or_ignores():
    spec, cfg = _spec_and_cfg()
    fm, im, caps = _batch(spec, 6, 11, 7)
    dec = cdec.Decoder(spec, _params(cfg, 3), DEV)
    with pytest.raises(ValueError, match='do not combine'):
        dec.train_step(dev(fm), dev(im), caps, rewards=np.ones(6, np.float32), soft=SOFT)
    with pytest.raises(ValueError, match='without a teacher table'):
        dec.train_step(dev(fm), dev(im), caps, soft=SOFT)
    hard = dec.train_step(dev(fm), dev(im), caps, training=False)
    loss = float(hard['loss'])
    same = dec.train_step(dev(fm), dev(im), caps, training=False, soft=SOFT)             # evaluation ignores the record
    assert float(same['loss']) == loss == float(same['nll']) and len(dec._ctx) == 1
    off = dec.train_step(dev(fm), dev(im), caps, training=False, soft=cdec.SoftTargets())
    assert float(off['loss']) == loss and len(dec._ctx) == 1


# ================================================================================ the command line ===================
def _run(module_path, argv):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('cli_soft_' + os.path.basename(module_path)[:-3], module_path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(argv)


def test_label_smoothing_then_distillation_cli(tmp_path, capsys):
    """train.py --label_smoothing 0.1 for a few steps, then a second run distilled from that checkpoint: finite losses with
    dec_nll logged beside them, run directories with the suffixes, config.pkl with the fields, and infer.py decodes the
    distilled model without any new flag"""
    import glob
    import json
    import os
    import re
    from comic_amd import configuration as conf
    from tests import tiny_dataset
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ds = tiny_dataset.make(str(tmp_path / 'mscoco'), n_train=16, n_valid=4, n_test=4)
    logs = str(tmp_path / 'experiments')
    common = ['--dataset_dir', ds, '--log_root', logs, '--cnn_name', 'inception_v3', '--cnn_fm_attention', 'Mixed_7c',
              '--cnn_input_size', '139,139', '--batch_size_eval', '4', '--rnn_size', '128', '--rnn_word_size', '64',
              '--train_mode', 'decoder', '--batch_size_train', '8', '--max_epoch', '2']
    train = os.path.join(root, 'src', 'train.py')

    def logged():
        out = capsys.readouterr().out
        assert not glob.glob(os.path.join(logs, 'mscoco', 'error__*')), out[-3000:]
        ppl = [float(x) for x in re.findall(r'Perplexity\s+([0-9.eE+-]+|nan|inf)', out)]
        nll = [float(x) for x in re.findall(r'dec_nll\s+([0-9.eE+-]+|nan|inf)', out)]
        assert len(ppl) >= 2 and len(nll) == len(ppl) and np.isfinite(ppl).all() and np.isfinite(nll).all(), out[-3000:]
        return ppl, nll
    _run(train, common + ['--label_smoothing', '0.1'])
    logged()
    name = 'radix_b256_add_LN_softmax_h8_tie_lstm'
    ls_dir = os.path.join(logs, 'mscoco', name + '_ls0.1_run_01')
    c = conf.load_config(os.path.join(ls_dir, 'config.pkl'))
    assert c.label_smoothing == 0.1 and not hasattr(c, 'distill_checkpoints')
    teacher = sorted(glob.glob(os.path.join(ls_dir, 'model_compact-*.npz')))[-1]
    _run(train, common + ['--distill_checkpoints', teacher, '--distill_weight', '0.5', '--distill_top_k', '8',
                          '--distill_temperature', '2'])
    ppl, nll = logged()
    assert any(abs(np.log(p) - n) > 1e-3 for p, n in zip(ppl, nll))                  # the soft loss is not the hard one
    kd_dir = os.path.join(logs, 'mscoco', name + '_kd0.5_k8_t2_run_01')
    c = conf.load_config(os.path.join(kd_dir, 'config.pkl'))
    assert (c.distill_checkpoints, c.distill_weight, c.distill_top_k, c.distill_temperature) == (teacher, 0.5, 8, 2.0)
    assert not hasattr(c, 'label_smoothing')
    _run(os.path.join(root, 'src', 'infer.py'), ['--infer_checkpoints_dir', kd_dir, '--dataset_dir', ds, '--infer_set', 'test',
                                                 '--batch_size_infer', '2', '--get_metric_score', ''])
    caps = glob.glob(os.path.join(kd_dir, 'infer_test_beam_3_lpen_0.0', 'captions___*.json'))
    assert caps and len(json.load(open(caps[0]))) == 4
