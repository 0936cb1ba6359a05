"""--cnn_dtype f16: the frozen encoder on IEEE half storage and the f16 matrix cores (COMIC_F16), against the fp32
oracle and against the bf16 plan on the same inputs and weights."""
import glob
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import comic_amd._lib as L
from comic_amd import decoder as cdec, nets, trainer
from oracle import cnn_ref
from tests.gpu_util import DEV, F32_RTOL, assert_close, dev, rel_err, sync

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16_TOL = 5e-3           # priced worst case on the oracle: 2.3e-3
F16_EMU_TOL = 2.5e-3     # the product plan against the f16-storage emulation of the oracle (measured 1.8e-3: see the test)
# end points of the product plan (pool after projection, fused pools): where its rewrites act, and the blocks behind them
PRODUCT_END_POINTS = ('MaxPool_3a_3x3', 'Conv2d_3b_1x1', 'Conv2d_4a_3x3', 'Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6a',
                      'Mixed_6c', 'Mixed_6e', 'Mixed_7a', 'Mixed_7b')


def _product_plan(size, **kw):
    """The frozen encoder's plan as the product builds it (model.py, bench.py)."""
    return nets.CnnPlan('inception_v3', (size, size), pool_after_projection=True, fuse_pools=True, **kw)


@pytest.fixture(scope='module')
def cnn_params():
    return cnn_ref.randomize_bn(cnn_ref.init_params(0, 224), seed=1)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t


@pytest.mark.parametrize('size,B', [(224, 2), (299, 2), (224, 97)])
def test_inception_v3_forward_f16(cnn_params, size, B):
    """Every end point the bf16 parity test checks, the feature map and the pooled embedding within 5e-3 of the fp32
    oracle; Mixed_7c and the embedding at most 0.3x the bf16 plan's deviation on the same inputs (a plan that quietly ran
    bf16 would fail here).  B = 97 is at or above CHAIN_MIN_BATCH (fused chains), B = 2 below it (the sibling plan).
    The embedding's ratio bar is 0.35: measured 0.315 at 224 / B = 2 (1.34e-3 against 4.25e-3), 0.22-0.28 elsewhere."""
    params = cnn_params if size == 224 else cnn_ref.randomize_bn(cnn_ref.init_params(0, size), seed=1)
    x = np.random.default_rng(7 + size + B).uniform(-1, 1, (B, size, size, 3)).astype(np.float32)
    plan = nets.CnnPlan('inception_v3', (size, size))
    assert (B >= plan.CHAIN_MIN_BATCH) == (B == 97)
    e16 = nets.CnnEncoder(plan, params, B, 'f16', DEV)
    eb = nets.CnnEncoder(plan, params, B, 'bf16', DEV)
    assert e16.dcode == 2 and any(b.dtype == torch.float16 for b in e16.bufs)
    assert not any(b.dtype == torch.bfloat16 for b in e16.bufs)
    im, fm = (t.clone() for t in e16.forward(dev(x)))
    imb, fmb = (t.clone() for t in eb.forward(dev(x)))
    sync()
    n = 2                                                    # images checked against the oracle
    net_ref, ep = cnn_ref.inception_v3(params, x[:n], act_dtype='f32')
    for name in ('Conv2d_1a_3x3', 'Conv2d_2b_3x3', 'MaxPool_5a_3x3', 'Mixed_5b', 'Mixed_5d', 'Mixed_6a',
                 'Mixed_6e', 'Mixed_7a', 'Mixed_7b'):
        got = e16.end_point(name)
        assert_close(got[:n].float().cpu().numpy(), ep[name], F16_TOL, name + ' f16')
    hw = fm.shape[1]
    s = int(round(hw ** 0.5))
    ref7 = ep['Mixed_7c']
    e_fm = rel_err(fm[:n].cpu().numpy().reshape(n, s, s, 2048), ref7)
    e_im = rel_err(im[:n].cpu().numpy(), net_ref.reshape(n, -1))
    b_fm = rel_err(fmb[:n].cpu().numpy().reshape(n, s, s, 2048), ref7)
    b_im = rel_err(imb[:n].cpu().numpy(), net_ref.reshape(n, -1))
    print('inception_v3 %d B=%d: f16 fm %.2e im %.2e | bf16 fm %.2e im %.2e' % (size, B, e_fm, e_im, b_fm, b_im))
    assert e_fm <= F16_TOL and e_im <= F16_TOL, (e_fm, e_im)
    assert e_fm <= 0.3 * b_fm and e_im <= 0.35 * b_im, (e_fm, b_fm, e_im, b_im)


def test_inception_v1_forward_f16():
    B = 2
    params = cnn_ref.randomize_bn(cnn_ref.init_params_v1(0), seed=1)
    x = np.random.default_rng(3).uniform(-1, 1, (B, 224, 224, 3)).astype(np.float32)
    plan = nets.CnnPlan('inception_v1', (224, 224), 'Mixed_4f')
    e16 = nets.CnnEncoder(plan, params, B, 'f16', DEV)
    eb = nets.CnnEncoder(plan, params, B, 'bf16', DEV)
    im, fm = (t.clone() for t in e16.forward(dev(x)))
    imb, fmb = (t.clone() for t in eb.forward(dev(x)))
    sync()
    net_ref, ep = cnn_ref.inception_v1(params, x, act_dtype='f32')
    assert fm.dtype == torch.float32 and fm.shape == (B, 196, 832)     # the inner end point is handed over in fp32
    for name in ('Conv2d_1a_7x7', 'MaxPool_2a_3x3', 'Conv2d_2c_3x3', 'Mixed_3c', 'Mixed_4b', 'Mixed_4e', 'Mixed_5b'):
        got = e16.end_point(name).float().cpu().numpy()
        assert_close(got[..., :ep[name].shape[-1]], ep[name], F16_TOL, name + ' f16')
    e_fm = rel_err(fm.cpu().numpy().reshape(B, 14, 14, 832), ep['Mixed_4f'])
    e_im = rel_err(im.cpu().numpy(), net_ref.reshape(B, -1))
    b_fm = rel_err(fmb.cpu().numpy().reshape(B, 14, 14, 832), ep['Mixed_4f'])
    b_im = rel_err(imb.cpu().numpy(), net_ref.reshape(B, -1))
    print('inception_v1: f16 fm %.2e im %.2e | bf16 fm %.2e im %.2e' % (e_fm, e_im, b_fm, b_im))
    assert e_fm <= F16_TOL and e_im <= F16_TOL
    assert e_fm <= 0.3 * b_fm and e_im <= 0.3 * b_im


@pytest.mark.parametrize('B', [3, 70])
def test_f16_fused_chains_graph_and_autotune_keep_the_bits(cnn_params, B):
    """The fused-chain plan gives the bits of the plan with one launch per conv depth; graph replay equals eager; the
    autotuner's tile choices keep the bits."""
    x = np.random.default_rng(31 + B).uniform(-1, 1, (B, 224, 224, 3)).astype(np.float32)
    sep = nets.CnnPlan('inception_v3', (224, 224), pool_after_projection=True, fuse_pools=True, fuse_chains=False)
    fus = nets.CnnPlan('inception_v3', (224, 224), pool_after_projection=True, fuse_pools=True, fuse_chains=True)
    e0 = nets.CnnEncoder(sep, cnn_params, B, 'f16', DEV)
    e1 = nets.CnnEncoder(fus, cnn_params, B, 'f16', DEV, weights_from=e0)
    im0, fm0 = (t.clone() for t in e0.forward(dev(x)))
    im1, fm1 = (t.clone() for t in e1.forward(dev(x)))
    sync()
    for name in ('Mixed_6b', 'Mixed_6e', 'Mixed_7a'):
        assert torch.equal(_bits(e1.end_point(name)), _bits(e0.end_point(name))), name
    assert torch.equal(fm1, fm0) and torch.equal(im1, im0)
    for _ in range(2):
        im2, fm2 = e1.forward(dev(x), use_graph=True)
    sync()
    assert torch.equal(fm2, fm0) and torch.equal(im2, im0)
    e0.autotune(reps=1)
    im3, fm3 = e0.forward(dev(x))
    sync()
    assert torch.equal(fm3, fm0) and torch.equal(im3, im0)


def test_f16_tile_variants_give_the_same_bits(cnn_params):
    """Every tile id a representative conv accepts (im2col, patch-resident, image-resident) gives the same bits on f16."""
    B = 4
    x = np.random.default_rng(5).uniform(-1, 1, (B, 224, 224, 3)).astype(np.float32)
    plan = nets.CnnPlan('inception_v3', (224, 224))
    enc = nets.CnnEncoder(plan, cnn_params, B, 'f16', DEV)
    enc.forward(dev(x))
    sync()
    lib, st = L.load(), L.stream_ptr()
    picked = []
    for want in ((3, 3, 1, 64), (1, 1, 1, 288), (1, 7, 1, 128), (3, 3, 2, 288)):
        for i, o in enumerate(plan.ops):
            if o['kind'] == 0 and (o['KH'], o['KW'], o['SH'], o['Cin']) == want and o.get('group', 0) <= 0:
                picked.append(i)
                break
    assert picked
    ids = list(range(1, L.CONV_TILES + 1)) + [L.IMG_TILE]
    n_ok = 0
    for i in picked:
        o = plan.ops[i]
        src, dst = enc.bufs[o['src']], enc.bufs[o['dst']]
        op = L.CnnOp()
        for k, v in o.items():
            if k not in ('depth', 'branch', 'block_in'):
                setattr(op, k, v)
        op.group, op.lane = 0, 0
        ref = None
        for t in ids:
            if t in (L.WS_TILE,):
                continue
            op.tile = t
            dst.zero_()
            rc = lib.comic_conv2d_bn_relu(C_ref(op), src.data_ptr(), src.shape[3], dst.data_ptr(), dst.shape[3],
                                          C_ref(enc._wt[o['weight']]), B, enc.dcode, st)
            if rc != 0:
                continue          # tile not eligible for this shape
            sync()
            got = dst.clone()
            if ref is None:
                ref = got
            else:
                assert torch.equal(_bits(got), _bits(ref)), (i, t)
            n_ok += 1
    assert n_ok >= 8


def C_ref(x):
    import ctypes
    return ctypes.byref(x)


def test_f16_refresh_weights_matches_a_fresh_encoder(cnn_params):
    B = 3
    x = np.random.default_rng(9).uniform(-1, 1, (B, 224, 224, 3)).astype(np.float32)
    plan = nets.CnnPlan('inception_v3', (224, 224), pool_after_projection=True, fuse_pools=True)
    other = cnn_ref.randomize_bn(cnn_ref.init_params(3, 224), seed=4)
    e0 = nets.CnnEncoder(plan, other, B, 'f16', DEV)
    e0.load_params(cnn_params)          # masters replaced, plan copy / fragment copy re-derived (comic_cnn_refresh_weights)
    e1 = nets.CnnEncoder(plan, cnn_params, B, 'f16', DEV)
    sync()
    assert torch.equal(_bits(e0.w_plan), _bits(e1.w_plan)) and torch.equal(_bits(e0.w_frag), _bits(e1.w_frag))
    im0, fm0 = (t.clone() for t in e0.forward(dev(x)))
    im1, fm1 = e1.forward(dev(x))
    sync()
    assert torch.equal(fm0, fm1) and torch.equal(im0, im1)


def test_f16_encoder_is_forward_only(cnn_params):
    plan = nets.CnnPlan('inception_v3', (224, 224))
    enc = nets.CnnEncoder(plan, cnn_params, 2, 'f16', DEV)
    with pytest.raises(ValueError, match='forward-only'):
        enc.enable_training()
    with pytest.raises(ValueError):
        nets.CnnEncoder(nets.CnnPlan('inception_v3', (224, 224), x3=True), cnn_params, 2, 'f16', DEV)


def test_f16_xe_step_against_the_fp32_plan(cnn_params):
    """One XE step at batch 64 / 224 (dropout off, same weights): the f16 plan's deviation from the fp32 plan, and the
    bf16 plan's for comparison.  The logits bar is 1e-2: the forecast was 6e-3, the device measured 7.6e-3 (bf16: 3.9e-2);
    feature map 1.9e-3 (<= 4e-3) and gradients 1.8e-2 (<= 5e-2) met their forecast bars."""
    B, IMG = 64, 224
    rng = np.random.default_rng(11)
    spec = cdec.DecoderSpec()
    tr32 = trainer.CaptionTrainer(cnn_params, spec, None, B, (IMG, IMG), 'f32', DEV, seed=8,
                                  plan=nets.CnnPlan('inception_v3', (IMG, IMG)))
    p_same = tr32.decoder.params.to_numpy()
    plan = nets.CnnPlan('inception_v3', (IMG, IMG), pool_after_projection=True, fuse_pools=True)
    imgs = torch.from_numpy(rng.uniform(-1, 1, (B, IMG, IMG, 3)).astype(np.float32)).to(DEV)
    caps = np.full((B, 12), -1, np.int64)
    for b in range(B):
        n = 3 + b % 8
        caps[b, 0] = 256
        caps[b, 1:n] = rng.integers(0, 256, n - 1)
        caps[b, n] = 257
    got = {}
    for name, dt in (('f32', None), ('bf16', 'bf16'), ('f16', 'f16')):
        t = tr32 if dt is None else trainer.CaptionTrainer(cnn_params, spec, p_same, B, (IMG, IMG), dt, DEV, seed=8, plan=plan)
        im_e, fm_e = t.encoder.forward(imgs, use_graph=False)
        r = t.decoder.train_step(fm_e, im_e, caps, training=False)
        sync()
        got[name] = dict(fm=fm_e.float().cpu().numpy(), logits=r['logits'].cpu().numpy(), grads=t.decoder.grads.to_numpy())
        if dt is not None:
            del t
    dev_rel = {}
    for name in ('bf16', 'f16'):
        g = got[name]
        dev_rel[name] = dict(feature_map=rel_err(g['fm'], got['f32']['fm']), logits=rel_err(g['logits'], got['f32']['logits']),
                             grad_max=max(rel_err(g['grads'][k], got['f32']['grads'][k]) for k in got['f32']['grads']))
    print('xe step deviation from the fp32 plan:', json.dumps(dev_rel))
    f, b = dev_rel['f16'], dev_rel['bf16']
    assert f['feature_map'] <= 4e-3 and f['logits'] <= 1e-2 and f['grad_max'] <= 5e-2, f
    for k in f:
        assert f[k] <= 0.35 * b[k], (k, f, b)


def _run(module_path, argv):
    spec = importlib.util.spec_from_file_location('cli_' + os.path.basename(module_path)[:-3], module_path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(argv)


def test_cli_chain_with_f16(tmp_path):
    """decoder (f16) -> cnn_finetune (bf16) -> scst (f16) -> infer from the SCST run; infer --cnn_dtype f16 on the
    bf16-trained cnn_finetune run."""
    from tests import tiny_dataset
    from comic_amd import configuration as conf
    ds = tiny_dataset.make(str(tmp_path / 'mscoco'), n_train=16, n_valid=4, n_test=4)      # SCST batches are 10 images
    logs = str(tmp_path / 'experiments')
    common = ['--dataset_dir', ds, '--log_root', logs, '--cnn_name', 'inception_v3', '--cnn_fm_attention', 'Mixed_7c',
              '--cnn_input_size', '139,139', '--batch_size_eval', '4', '--rnn_size', '128', '--rnn_word_size', '64']
    train, infer = os.path.join(ROOT, 'src', 'train.py'), os.path.join(ROOT, 'src', 'infer.py')

    def no_errors():
        errs = glob.glob(os.path.join(logs, 'mscoco', 'error__*'))
        assert not errs, open(errs[0]).read()

    _run(train, common + ['--train_mode', 'decoder', '--batch_size_train', '4', '--max_epoch', '1', '--cnn_dtype', 'f16'])
    no_errors()
    run_dir = os.path.join(logs, 'mscoco', 'radix_b256_add_LN_softmax_h8_tie_lstm_run_01')
    assert conf.load_config(os.path.join(run_dir, 'config.pkl')).cnn_dtype == 'f16'
    _run(train, common + ['--train_mode', 'cnn_finetune', '--batch_size_train', '4', '--max_epoch', '1', '--cnn_dtype', 'bf16'])
    no_errors()
    ft_dir = run_dir.replace('_run_01', '_cnnFT_run_01')
    assert conf.load_config(os.path.join(ft_dir, 'config.pkl')).cnn_dtype == 'bf16'
    _run(train, common + ['--train_mode', 'scst', '--max_epoch', '1', '--scst_beam_size', '2', '--cnn_dtype', 'f16'])
    no_errors()
    scst_dir = glob.glob(os.path.join(logs, 'mscoco', '*_cnnFT_SCST_beam_2_*'))[0]
    assert conf.load_config(os.path.join(scst_dir, 'config.pkl')).cnn_dtype == 'f16'
    for d, extra in ((scst_dir, []), (ft_dir, ['--cnn_dtype', 'f16'])):
        _run(infer, ['--infer_checkpoints_dir', d, '--dataset_dir', ds, '--infer_set', 'test', '--batch_size_infer', '2',
                     '--get_metric_score', ''] + extra)
        caps = glob.glob(os.path.join(d, 'infer_test_beam_3_lpen_0.0', 'captions___*.json'))
        assert caps
        data = json.load(open(caps[0]))
        assert len(data) == 4 and all(set(x) == {'image_id', 'caption'} for x in data)


@pytest.mark.parametrize('size,B', [(224, 2), (224, 97), (299, 2)])
def test_inception_v3_product_plan_f16(cnn_params, size, B):
    """The f16 encoder on the plan train.py / infer.py --cnn_dtype f16 run (kind-9 stem stream, MaxPool_3a / 5a folded into
    the 1x1 convs behind them, the pool branches as projection then kind-7 average + BN + ReLU, fused chains at B = 97):
    every end point against the fp32 oracle at F16_TOL, and against the oracle's f16-storage emulation (act_dtype='f16')
    at the tighter F16_EMU_TOL.  Measured against the emulation: at most 1.8e-3 over these end points (Mixed_6e at 224;
    1.4e-3 or less at Mixed_7c and 4.8e-4 at the embedding; the emulation
    rounds the image and the stem filter, which the device reads in fp32, and differs in the order of the rounding of
    the pool branches).  B = 97: a permuted batch gives the permuted features bit for bit, the last partial pixel tile
    included, so every image is held to the two compared with the oracle."""
    params = cnn_params if size == 224 else cnn_ref.randomize_bn(cnn_ref.init_params(0, size), seed=1)
    x = np.random.default_rng(70 + size + B).uniform(-1, 1, (B, size, size, 3)).astype(np.float32)
    plan = _product_plan(size)
    assert plan.ops[0]['kind'] == (9 if size % 4 == 0 else 1) and sum(1 for o in plan.ops if o['kind'] == 7) == 9   # kind 9: W % 4 == 0
    # MaxPool_5a folded into the four 1x1s of Mixed_5b; MaxPool_3a into Conv2d_3b unless the kind-9 stem stream pools it
    assert sum(1 for o in plan.ops if o.get('flags', 0) & L.OP_POOLED_SRC) == (4 if size % 4 == 0 else 5)
    enc = nets.CnnEncoder(plan, params, B, 'f16', DEV)
    im, fm = (t.clone() for t in enc.forward(dev(x)))
    sync()
    n = 2
    net_ref, ep = cnn_ref.inception_v3(params, x[:n], act_dtype='f32')
    net_emu, ep_emu = cnn_ref.inception_v3(params, x[:n], act_dtype='f16')
    s = int(round(fm.shape[1] ** 0.5))
    worst = {}
    names = [k for k in PRODUCT_END_POINTS if k in plan.end_points]
    assert len(names) == len(PRODUCT_END_POINTS) - (0 if size % 4 == 0 else 1)     # 299: MaxPool_3a is never materialised
    for name in names:
        got = enc.end_point(name)[:n].float().cpu().numpy()
        assert_close(got, ep[name], F16_TOL, name + ' f16 product plan')
        worst[name] = rel_err(got, ep_emu[name])
    worst['Mixed_7c'] = rel_err(fm[:n].cpu().numpy().reshape(n, s, s, 2048), ep_emu['Mixed_7c'])
    worst['embedding'] = rel_err(im[:n].cpu().numpy(), net_emu.reshape(n, -1))
    assert_close(fm[:n].cpu().numpy().reshape(n, s, s, 2048), ep['Mixed_7c'], F16_TOL, 'Mixed_7c f16 product plan')
    assert_close(im[:n].cpu().numpy(), net_ref.reshape(n, -1), F16_TOL, 'embedding f16 product plan')
    print('product plan %d B=%d, deviation from the f16 emulation: %s' % (size, B, json.dumps({k: float('%.3g' % v) for k, v in worst.items()})))
    assert max(worst.values()) <= F16_EMU_TOL, worst
    if B == 97:
        perm = np.random.default_rng(1).permutation(B)
        im2, fm2 = enc.forward(dev(x[perm]))
        sync()
        assert torch.equal(fm2, fm[perm]) and torch.equal(im2, im[perm])


def test_f16_fused_pools_weight_stationary_1x1(cnn_params):
    """f16 counterpart of the bf16 weight-stationary test: the thin 1x1 groups of Mixed_5b-d forced onto tile 54, the
    pooled-source 1x1s, the row-walking kind-7 kernel -- bit for bit against the plain forward-only plan with every conv on
    im2col tile 3 (same k order per accumulator, exact max), and against the fp32 oracle."""
    B = 3
    x = np.random.default_rng(12).uniform(-1, 1, (B, 224, 224, 3)).astype(np.float32)
    pa = nets.CnnPlan('inception_v3', (224, 224), pool_after_projection=True, fuse_chains=False)
    pb = _product_plan(224, fuse_chains=True)
    ea = nets.CnnEncoder(pa, cnn_params, B, 'f16', DEV)
    eb = nets.CnnEncoder(pb, cnn_params, B, 'f16', DEV, weights_from=ea)
    for i, o in enumerate(pa.ops):
        if o['kind'] == 0:
            ea._ops[i].tile = 3
    n_ws = 0
    for i, o in enumerate(pb.ops):
        if o['kind'] == 0 and o['KH'] == 1 and o['Cin'] in (256, 288) and o['Ho'] == 25:
            eb._ops[i].tile = L.WS_TILE
            n_ws += 1
    assert n_ws >= 6
    for e, plan in ((ea, pa), (eb, pb)):
        for i, o in enumerate(plan.ops):
            if o['kind'] == 7:
                e._ops[i].tile = 1
    ea._build_group_args()
    eb._build_group_args()
    ima, fma = (t.clone() for t in ea.forward(dev(x)))
    imb, fmb = eb.forward(dev(x))
    sync()
    net_ref, ep = cnn_ref.inception_v3(cnn_params, x[:2], act_dtype='f32')
    for name in ('MaxPool_3a_3x3', 'Conv2d_3b_1x1', 'Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6c', 'Mixed_7b'):
        assert_close(eb.end_point(name)[:2].float().cpu().numpy(), ep[name], F16_TOL, name)
        assert torch.equal(_bits(eb.end_point(name)), _bits(ea.end_point(name))), name
    assert torch.equal(fma, fmb) and torch.equal(ima, imb)


def test_f16_grouped_branch_launch_is_bit_identical():
    """f16: comic_cnn_forward_grouped (one launch per depth of an Inception block) against the op-by-op executor, every
    end point bit for bit at a ragged batch, eager and replayed from a graph."""
    params = cnn_ref.randomize_bn(cnn_ref.init_params(0, 224), seed=2)
    x = np.random.default_rng(7).uniform(-1, 1, (5, 224, 224, 3)).astype(np.float32)
    single = nets.CnnEncoder(nets.CnnPlan('inception_v3', (224, 224), group_branches=False), params, 5, 'f16', DEV)
    grouped = nets.CnnEncoder(nets.CnnPlan('inception_v3', (224, 224), group_branches=True), params, 5, 'f16', DEV)
    assert grouped._group_args is not None and single._group_args is None
    im0, fm0 = (t.clone() for t in single.forward(dev(x)))
    im1, fm1 = grouped.forward(dev(x))
    sync()
    for name in single.plan.end_points:
        assert torch.equal(_bits(single.end_point(name)), _bits(grouped.end_point(name))), name
    assert torch.equal(fm0, fm1) and torch.equal(im0, im1)
    for _ in range(2):
        im2, fm2 = grouped.forward(dev(x), use_graph=True)
    sync()
    assert torch.equal(fm0, fm2) and torch.equal(im0, im2)


def test_f16_walk_tiles_give_the_bits_of_the_one_tile_launch(cnn_params):
    """f16: tile ids 56..61 (one workgroup per pixel tile walks over the out-channel tiles of every member of a shared-input
    1x1 group) against the same groups on tile 44, the whole forward bit for bit."""
    B = 3
    x = np.random.default_rng(10).uniform(-1, 1, (B, 224, 224, 3)).astype(np.float32)
    plan = nets.CnnPlan('inception_v3', (224, 224), pool_after_projection=True, fuse_chains=False)
    enc = nets.CnnEncoder(plan, cnn_params, B, 'f16', DEV)
    heads = [i for i, o in enumerate(plan.ops) if o['kind'] == 0 and o.get('group', 0) and o['KH'] == 1 and o['KW'] == 1 and o['depth'] == 0
             and (i == 0 or plan.ops[i - 1].get('group', 0) != o['group'])]
    assert len(heads) >= 9

    def forward_with(tile):
        for i in heads:
            enc._ops[i].tile = tile
        enc._build_group_args(); enc._drop_graphs()
        im, fm = enc.forward(dev(x))
        sync()
        return im.clone(), fm.clone()
    im0, fm0 = forward_with(44)
    for tile in (56, 57, 58, 59, 60, 61):
        im1, fm1 = forward_with(tile)
        assert torch.equal(fm1, fm0) and torch.equal(im1, im0), 'walk tile %d differs' % tile


def test_inception_v1_stem_wide_kernel_f16():
    """Inception-V1's Conv2d_1a_7x7 (7x7 / 2 SAME, 3 -> 64) on an f16 plan runs on conv_stem_wide_kernel (16-bit plans only):
    the stem's output against float64 on the fp32 image and filter, rounded once to f16, at the fp32 bar; the whole
    forward against the fp32 oracle at F16_TOL; the direct stem kernel (tile 1) within the same fp32 bar."""
    B = 3
    params = cnn_ref.randomize_bn(cnn_ref.init_params_v1(0), seed=1)
    x = np.random.default_rng(4).uniform(-1, 1, (B, 224, 224, 3)).astype(np.float32)
    plan = nets.CnnPlan('inception_v1', (224, 224), 'Mixed_4f')
    stem = [i for i, o in enumerate(plan.ops) if o['kind'] == 1]
    assert len(stem) == 1 and (plan.ops[stem[0]]['KH'], plan.ops[stem[0]]['Cout']) == (7, 64) and not plan.ops[stem[0]].get('tile')
    enc = nets.CnnEncoder(plan, params, B, 'f16', DEV)
    im, fm = (t.clone() for t in enc.forward(dev(x)))
    y = enc.end_point('Conv2d_1a_7x7').float().cpu().numpy()
    sync()
    name = [k for k in params if k.endswith('Conv2d_1a_7x7/weights')][0]
    pre = name[:-len('weights')]
    ref = cnn_ref.conv2d(x.astype(np.float64), params[name].astype(np.float64), 2, 'SAME')
    ref = (ref - params[pre + 'BatchNorm/moving_mean']) / np.sqrt(params[pre + 'BatchNorm/moving_variance'].astype(np.float64)
                                                                  + cnn_ref.BN_EPS) + params[pre + 'BatchNorm/beta']
    ref = cnn_ref.f16_round(np.maximum(ref, 0))
    assert_close(y[..., :64], ref, F32_RTOL, 'Conv2d_1a_7x7 f16 (wide stem kernel)', elementwise=True)
    net_ref, ep = cnn_ref.inception_v1(params, x[:2], act_dtype='f32')
    for n_ in ('MaxPool_2a_3x3', 'Conv2d_2c_3x3', 'Mixed_3c', 'Mixed_4e'):
        got = enc.end_point(n_)[:2].float().cpu().numpy()
        assert_close(got[..., :ep[n_].shape[-1]], ep[n_], F16_TOL, n_ + ' f16')
    assert_close(fm[:2].cpu().numpy().reshape(2, 14, 14, 832), ep['Mixed_4f'], F16_TOL, 'Mixed_4f f16')
    enc._ops[stem[0]].tile = 1
    enc._drop_graphs()
    enc.forward(dev(x))
    sync()
    assert_close(enc.end_point('Conv2d_1a_7x7').float().cpu().numpy()[..., :64], ref, F32_RTOL, 'Conv2d_1a_7x7 f16 (direct)',
                 elementwise=True)
