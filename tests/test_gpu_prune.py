"""`--prune_sparsity` on the GPU: the mask event (comic_prune_select) against tests/prune_ref.py bit for bit, the masked
optimiser launches against their unmasked twins, the ranges of the chunked gradient exchange across an event, the trajectory
through training steps for both scopes, with the shadow and with the clip, and the CLIs."""
import glob
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import comic_amd._lib as L
from comic_amd import checkpoint as ckpt, decoder as cdec, optim, prune
from tests import prune_ref
from tests.gpu_util import DEV, assert_close, dev, lib, stream, sync

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64
SENTINEL = 7.5


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---- 1. the selection ----------------------------------------------------------------------------------------------------
SIZES = (1, 31, 32, 33, 255, 8192, 8193, 100003)
DENSE = 4                               # SIZES[4] (255) is not prunable: it lies between two prunable segments
MAGNITUDES = np.array([0.0, -0.0, 1e-40, 0.25, -0.25, 3.0, -3.0], np.float32)       # five magnitudes: +-0, a denormal, +-x pairs


def _flat_case(kind, n_groups):
    """Buffers laid out like FlatParams.  The padding holds a sentinel whose magnitude lies below every (non-zero) weight:
    a kernel that counts or touches padding picks it first."""
    rng = np.random.default_rng(len(kind) + 10 * n_groups)
    offs, total = prune_ref.layout(SIZES)
    tiny = np.float32(1e-45) if kind == 'ties' else np.float32(1e-30)
    w = np.full(total, tiny, np.float32)
    for off, n in zip(offs, SIZES):
        w[off:off + n] = rng.choice(MAGNITUDES, n) if kind == 'ties' else rng.standard_normal(n).astype(np.float32)
    if kind == 'normal':
        assert np.abs(w[w != tiny]).min() > tiny
    others = [(rng.standard_normal(total) + 3).astype(np.float32) for _ in range(3)]            # m, v, shadow: never zero
    prunable = [i for i in range(len(SIZES)) if i != DENSE]
    segments = [(offs[i], SIZES[i], j % n_groups) for j, i in enumerate(prunable)]             # groups interleave
    return w, others, segments, total


class _Event:
    def __init__(self, total, segments, n_groups):
        self.total, self.n_seg, self.n_groups = total, len(segments), n_groups
        self.table = dev(np.asarray(segments, np.int64))
        ws = lib().comic_prune_workspace_bytes(total, self.n_seg, n_groups)
        assert ws > 0
        self.ws = torch.empty(ws + PAD, dtype=torch.uint8, device=DEV).fill_(0xA5)
        self.ws_bytes = ws

    def run(self, bufs, words, targets, shadow=True):
        """bufs: host w, m, v, shadow; words: host uint32 -> the five arrays after the event."""
        d = [dev(b) for b in bufs]
        dw = dev(words.view(np.int32))
        k = dev(np.asarray(targets, np.int64))
        L.check(lib().comic_prune_select(d[0].data_ptr(), dw.data_ptr(), self.total, self.table.data_ptr(), self.n_seg,
                                         k.data_ptr(), self.n_groups, d[1].data_ptr(), d[2].data_ptr(),
                                         d[3].data_ptr() if shadow else None, self.ws.data_ptr(), self.ws_bytes, stream()),
                'prune_select')
        sync()
        assert bool((self.ws[self.ws_bytes:] == 0xA5).all())                # nothing behind the stated workspace
        return [x.cpu().numpy() for x in d], dw.cpu().numpy().view(np.uint32)


def _targets(kind, sizes):
    mid = [n * 3 // 7 for n in sizes]
    per = {'zero': [0] * len(sizes), 'one': [1] * len(sizes), 'all_but_one': [n - 1 for n in sizes], 'all': list(sizes),
           'middle': mid}[kind]
    # several groups: not the same edge in every group
    if len(sizes) > 1 and kind != 'middle':
        per[1] = mid[1]
    return per


@pytest.mark.parametrize('target', ['zero', 'one', 'all_but_one', 'all', 'middle'])
@pytest.mark.parametrize('n_groups', [1, 3])
@pytest.mark.parametrize('kind', ['normal', 'ties'])
def test_select_equals_the_reference_bit_for_bit(kind, n_groups, target):
    w, others, segments, total = _flat_case(kind, n_groups)
    sizes = [sum(n for _, n, g in segments if g == gg) for gg in range(n_groups)]
    ev = _Event(total, segments, n_groups)
    live = np.ones(total, bool)
    bufs = [w] + others
    first = _targets(target, sizes)
    # event 2 asks for less than is pruned (nothing may change), event 3 for more
    plan = [first, [max(0, k - 1) for k in first], [min(n, k + 1 + (n - k) // 3) for k, n in zip(first, sizes)]]
    for i, targets in enumerate(plan):
        words = prune_ref.pack(live)
        want_live = prune_ref.select(bufs[0], live, segments, targets)
        want = prune_ref.apply(bufs, live, want_live)
        got, got_words = ev.run(bufs, words, targets)
        assert np.array_equal(got_words, prune_ref.pack(want_live)), (i, targets)
        for name, a, b in zip(('w', 'm', 'v', 'shadow'), got, want):
            assert _same_bits(a, b), (name, i)                              # +0.0f at the newly pruned, all else kept
        for g in range(n_groups):
            idx = prune_ref.group_indices(segments, g)
            assert int((~want_live[idx]).sum()) == max(int((~live[idx]).sum()), targets[g])
        if i == 1:
            assert np.array_equal(want_live, live)
        if i == 0:                                                          # a second run: the same bytes
            again, again_words = ev.run(bufs, words, targets)
            assert np.array_equal(again_words, got_words) and all(_same_bits(a, b) for a, b in zip(again, got))
        live, bufs = want_live, got
    dense = slice(prune_ref.layout(SIZES)[0][DENSE], prune_ref.layout(SIZES)[0][DENSE] + SIZES[DENSE])
    assert live[dense].all() and _same_bits(bufs[0][dense], w[dense])


def test_select_without_a_shadow_and_refusals():
    w, others, segments, total = _flat_case('ties', 3)
    ev = _Event(total, segments, 3)
    live = np.ones(total, bool)
    targets = [5, 4000, 60000]
    got, words = ev.run([w] + others, prune_ref.pack(live), targets, shadow=False)
    want_live = prune_ref.select(w, live, segments, targets)
    assert np.array_equal(words, prune_ref.pack(want_live)) and _same_bits(got[3], others[2])
    assert all(_same_bits(a, b) for a, b in zip(got[:3], prune_ref.apply([w] + others[:2], live, want_live)))
    # a table that points outside the buffer or at an unknown group is ignored, not followed
    odd = _Event(total, [(total - 10, 64, 0), (-64, 10, 0), (0, 1, 7), (64, 31, 0)], 1)
    got, words = odd.run([w] + others, prune_ref.pack(live), [31])
    want_live = live.copy()
    want_live[64:64 + 31] = False
    assert np.array_equal(words, prune_ref.pack(want_live))
    assert all(_same_bits(a, b) for a, b in zip(got, prune_ref.apply([w] + others, live, want_live)))
    d = [dev(np.zeros(64, np.float32)) for _ in range(4)]
    dw, tab, k = dev(np.full(2, -1, np.int32)), dev(np.asarray([(0, 64, 0)], np.int64)), dev(np.asarray([1], np.int64))
    ws = torch.empty(lib().comic_prune_workspace_bytes(64, 1, 1), dtype=torch.uint8, device=DEV)
    ok = [d[0].data_ptr(), dw.data_ptr(), 64, tab.data_ptr(), 1, k.data_ptr(), 1, d[1].data_ptr(), d[2].data_ptr(), None,
          ws.data_ptr(), ws.numel(), stream()]
    for pos, bad in ((0, None), (1, None), (3, None), (5, None), (7, None), (8, None), (10, None), (11, ws.numel() - 1),
                     (2, 0), (4, 0), (6, 0), (6, 2)):
        args = list(ok)
        args[pos] = bad
        with pytest.raises(L.ComicHipError):
            L.check(lib().comic_prune_select(*args))
    assert lib().comic_prune_workspace_bytes(0, 1, 1) == -1 and lib().comic_prune_workspace_bytes(64, 1, 2) == -1
    sync()
    assert _bits(dw).tolist() == [0xFFFFFFFF] * 2


def test_mask_buffer_and_mask_from_zeros():
    rng = np.random.default_rng(3)
    w, _, segments, total = _flat_case('ties', 1)
    dw = dev(w)
    words = dev(np.zeros(total // 32, np.int32))                            # overwritten: all ones, then the zeros cleared
    tab = dev(np.asarray(segments, np.int64))
    L.check(lib().comic_prune_mask_from_zeros(dw.data_ptr(), words.data_ptr(), total, tab.data_ptr(), len(segments), stream()))
    sync()
    want = np.ones(total, bool)
    for f, n, _ in segments:
        want[f:f + n] = w[f:f + n] != 0                                     # (-0.0 counts as zero)
    assert np.array_equal(_bits(words), prune_ref.pack(want)) and 0 < int((~want).sum()) < sum(SIZES)
    assert _same_bits(dw.cpu().numpy(), w)
    # mask_buffer: any first bit and length; +0.0f where the bit is clear, the rest and the tail untouched
    for first, n in ((0, total), (64 * 3, 1), (37, 1000), (8191, 8194)):
        x = (rng.standard_normal(n + PAD) - 5).astype(np.float32)
        dx = dev(x)
        L.check(lib().comic_prune_mask_buffer(dx.data_ptr(), words.data_ptr(), first, n, stream()))
        sync()
        ref = x.copy()
        ref[:n][~want[first:first + n]] = np.float32(0.0)
        assert _same_bits(dx.cpu().numpy(), ref), (first, n)
    for args in ((None, words.data_ptr(), 0, 8), (dw.data_ptr(), None, 0, 8), (dw.data_ptr(), words.data_ptr(), -1, 8),
                 (dw.data_ptr(), words.data_ptr(), 0, 0)):
        with pytest.raises(L.ComicHipError):
            L.check(lib().comic_prune_mask_buffer(*args, stream()))


# ---- 2. the masked launch ------------------------------------------------------------------------------------------------
def _padded(a):
    return dev(np.concatenate([a, np.full(PAD, SENTINEL, np.float32)]))


@pytest.mark.parametrize('first', [0, 64 * 3])
@pytest.mark.parametrize('n', [1, 255, 257, 100003])
@pytest.mark.parametrize('opt_name', ['adam', 'sgd'])
def test_masked_launch_is_its_twin_at_live_elements(opt_name, n, first):
    """Gated and EMA arithmetic, bit for bit, where the bit is set; +0.0f kept under a non-zero gradient where it is clear;
    the range starts at bit `first` of a larger mask; the tail is untouched; a set status word leaves all buffers."""
    rng = np.random.default_rng(n + first)
    live = rng.random(first + n + 40) < 0.5
    if n == 1:
        live[first] = True
    words = dev(prune_ref.pack(live).view(np.int32))
    here = live[first:first + n]
    w, s = (np.where(here, rng.standard_normal(n), 0.0).astype(np.float32) for _ in range(2))
    m = np.where(here, 0.1 * rng.standard_normal(n), 0.0).astype(np.float32)
    v = np.where(here, 0.1 * rng.random(n), 0.0).astype(np.float32)
    g = (rng.standard_normal(n) + 0.01).astype(np.float32)
    assert (g != 0).all()
    dg = dev(g)
    lr, l2, gs, omd = 1e-2, 1e-5, 0.5, 0.1
    lr_t = lr * math.sqrt(1 - 0.999 ** 3) / (1 - 0.9 ** 3)

    def twin(bufs, shadow):
        p = [b.data_ptr() for b in bufs]
        if opt_name == 'adam' and shadow is None:
            return lib().comic_adam_tf_gated(p[0], dg.data_ptr(), p[1], p[2], n, lr_t, 0.9, 0.999, 1e-2, l2, gs, None, stream())
        if opt_name == 'adam':
            return lib().comic_adam_tf_ema(p[0], dg.data_ptr(), p[1], p[2], n, lr_t, 0.9, 0.999, 1e-2, l2, gs, None,
                                           shadow.data_ptr(), omd, stream())
        if shadow is None:
            return lib().comic_momentum_tf_gated(p[0], dg.data_ptr(), p[1], n, lr, 0.9, l2, gs, None, stream())
        return lib().comic_momentum_tf_ema(p[0], dg.data_ptr(), p[1], n, lr, 0.9, l2, gs, None, shadow.data_ptr(), omd, stream())

    def masked(bufs, shadow, flag=None):
        p = [b.data_ptr() for b in bufs]
        sp, fp = shadow.data_ptr() if shadow is not None else None, flag.data_ptr() if flag is not None else None
        if opt_name == 'adam':
            return lib().comic_adam_tf_masked(p[0], dg.data_ptr(), p[1], p[2], n, lr_t, 0.9, 0.999, 1e-2, l2, gs, fp, sp,
                                              omd if shadow is not None else 0.0, words.data_ptr(), first, stream())
        return lib().comic_momentum_tf_masked(p[0], dg.data_ptr(), p[1], n, lr, 0.9, l2, gs, fp, sp,
                                              omd if shadow is not None else 0.0, words.data_ptr(), first, stream())

    for with_shadow in (False, True):
        a, b = [_padded(x) for x in (w, m, v)], [_padded(x) for x in (w, m, v)]
        sa, sb = (_padded(s), _padded(s)) if with_shadow else (None, None)
        L.check(twin(a, sa))
        L.check(masked(b, sb))
        sync()
        t_live = torch.from_numpy(here).to(DEV)
        for x, y, name in zip(a + [sa], b + [sb], ('w', 'm', 'v', 'shadow')):
            if x is None or (opt_name == 'sgd' and name == 'v'):
                continue
            assert torch.equal(x[:n][t_live], y[:n][t_live]), name                        # the twin's bits
            assert not _bits(y[:n][~t_live]).any(), name                                  # +0.0f stays
            assert bool((y[n:] == SENTINEL).all()), name
            if here.any() and (~here).any():
                assert not torch.equal(x[:n], y[:n]), name                                # the twin moved the pruned ones
        assert not torch.equal(b[0][:n], dev(w))
        flag = dev(np.ones(1, np.float32))
        before = [x.clone() for x in b + ([sb] if with_shadow else [])]
        L.check(masked(b, sb, flag))
        sync()
        assert all(torch.equal(x, y) for x, y in zip(before, b + ([sb] if with_shadow else [])))


def test_masked_entries_refuse_bad_arguments():
    x = [dev(np.zeros(8, np.float32)) for _ in range(5)]
    p = [t.data_ptr() for t in x]
    words = dev(np.full(1, -1, np.int32)).data_ptr()
    for mask, first, n, shadow, omd in ((None, 0, 8, None, 0.0), (words, -1, 8, None, 0.0), (words, 0, 0, None, 0.0),
                                        (words, 0, 8, p[4], 0.0), (words, 0, 8, p[4], 1.5), (words, 0, 8, p[4], float('nan'))):
        with pytest.raises(L.ComicHipError):
            L.check(lib().comic_adam_tf_masked(p[0], p[1], p[2], p[3], n, 1e-2, 0.9, 0.999, 1e-2, 0.0, 1.0, None, shadow, omd,
                                               mask, first, stream()))
        with pytest.raises(L.ComicHipError):
            L.check(lib().comic_momentum_tf_masked(p[0], p[1], p[2], n, 1e-2, 0.9, 0.0, 1.0, None, shadow, omd, mask, first,
                                                   stream()))
    for bad in (0, 2):
        args = [p[0], p[1], p[2], p[3], 8, 1e-2, 0.9, 0.999, 1e-2, 0.0, 1.0, None, None, 0.0, words, 0, stream()]
        args[bad] = None
        with pytest.raises(L.ComicHipError):
            L.check(lib().comic_adam_tf_masked(*args))
    sync()
    assert all(float(t.abs().max()) == 0.0 for t in x)


# ---- 3. ranges -----------------------------------------------------------------------------------------------------------
def _seeded_buffers(spec):
    g = torch.Generator(device='cpu').manual_seed(3)
    PP = cdec.FlatParams(spec.param_shapes(), DEV, status_tail=True)
    GG = cdec.FlatParams(spec.param_shapes(), DEV, status_tail=True)
    PP.data[:PP.numel].copy_(torch.randn(PP.numel, generator=g))
    GG.data[:GG.numel].copy_(torch.randn(GG.numel, generator=g))
    return PP, GG


@pytest.mark.parametrize('opt_name', ['adam', 'sgd'])
def test_masked_update_by_ranges_equals_one_launch_across_events(opt_name):
    """test_ema_update_by_ranges_equals_one_launch with a mask: events behind updates 1 and 2 (sparsity 0.4375, 0.5); the
    four ranges in reverse give the bits of the one-launch step in w, the slots, the shadow and the mask words."""
    from comic_amd.trainer import DataParallel
    spec = cdec.DecoderSpec(M=25, C=2048, Cg=2048)
    outs = []
    for mode in ('flat', 'ranges'):
        PP, GG = _seeded_buffers(spec)
        opt = optim.make_optimiser(opt_name, PP, ema_decay=0.9, prune=optim.PruneSpec(0.5, 0, 2, 1, 'layer'))
        assert all(f % 32 == 0 for f, _ in DataParallel.chunk_bounds(GG, 4))           # ranges start on a word boundary
        seen = []
        for step in range(3):
            if mode == 'flat':
                opt.step(GG, 1e-2, grad_scale=0.5)
            else:
                opt.step(GG, 1e-2, grad_scale=0.5, ranges=DataParallel.chunk_bounds(GG, 4)[::-1], before_range=seen.append)
        sync()
        assert mode == 'flat' or seen == [0, 1, 2, 3] * 3
        assert opt.mask.events == 2
        outs.append((PP.data.clone(), opt.m.data.clone(), opt.v.data.clone(), opt.ema.data.clone(), opt.mask.words.clone()))
        counts = opt.mask.pruned_counts()
        assert counts == {k: n // 2 for k, _, n, _ in opt.mask.segments}               # floor(0.5 n), exactly
        for k, off, n, _ in opt.mask.segments:
            dead = ~torch.from_numpy(prune_ref.unpack(opt.mask.to_numpy(), PP.numel)[off:off + n]).to(DEV)
            for buf in (PP, opt.m, opt.v, opt.ema):
                assert not _bits(buf.data[off:off + n][dead]).any(), k
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ---- 4. trajectory -------------------------------------------------------------------------------------------------------
def _trajectory_inputs(spec, B=4, T=6):
    rng = np.random.default_rng(5)
    fm = dev(rng.standard_normal((B, spec.M, spec.C)).astype(np.float32))
    im = dev(rng.standard_normal((B, spec.Cg)).astype(np.float32))
    caps = np.full((B, T), -1, np.int64)
    for b in range(B):
        n = T - 2 if b == 0 else int(rng.integers(1, T - 1))
        caps[b, 0], caps[b, 1:1 + n], caps[b, 1 + n] = spec.start_id, rng.integers(0, 256, n), spec.end_id
    return fm, im, caps


@pytest.mark.parametrize('scope,ema,clip', [('layer', 0.0, False), ('layer', 0.9, False), ('global', 0.0, False),
                                            ('global', 0.9, False), ('layer', 0.9, True)])
def test_prune_trajectory_through_training_steps(scope, ema, clip):
    """Eight training steps, events behind updates 2, 4, 6, 8 towards 0.5: after every event the device mask is the
    reference's on the device's own pre-event variables and every group holds exactly k_g pruned elements; after every step
    the pruned elements of w, m, v and the shadow are zero and the loss is finite.  With the clip: the clipped gradient is
    the reference's with the gradients of pruned weights as zero (1e-5, the bound of test_gradient_clipping_matches_oracle)."""
    from oracle import decoder_ref as dr
    spec = cdec.DecoderSpec(D=128, E=64, M=25, C=2048, Cg=2048)
    fm, im, caps = _trajectory_inputs(spec)
    dec = cdec.Decoder(spec, cdec.init_params(spec, 0), DEV, seed=3)
    clip_norm, l2 = 0.0, 1e-5
    if clip:            # a threshold between the variables' gradient norms: some are clipped, some are not
        dec.train_step(fm, im, caps, training=True, seed=70)
        sync()
        g0, w0 = dec.grads.to_numpy(), dec.params.to_numpy()
        clip_norm = float(np.median([np.linalg.norm((g0[k] + np.float32(l2) * w0[k]).astype(np.float64)) for k in g0]))
    opt = optim.AdamTF(dec.params, l2_decay=l2, clip_norm=clip_norm, ema_decay=ema,
                       prune=optim.PruneSpec(0.5, 2, 8, 2, scope))
    mask = opt.mask
    segs = [(f, n, g) for _, f, n, g in mask.segments]
    assert mask.n_groups == (len(segs) if scope == 'layer' else 1) and sum(mask.group_sizes) == sum(n for _, n, _ in segs)
    seen, run_event = [], mask.event

    def event(t, m, v, shadow):
        sync()
        pre_w, pre_live = dec.params.flat.cpu().numpy().copy(), prune_ref.unpack(mask.to_numpy(), mask.n_total)
        run_event(t, m, v, shadow)
        sync()
        targets = [prune.target_count(prune.prune_sparsity_at(t, 0.5, 2, 8), n) for n in mask.group_sizes]
        want = prune_ref.select(pre_w, pre_live, segs, targets)
        assert np.array_equal(mask.to_numpy(), prune_ref.pack(want)), t
        for g, k in enumerate(targets):
            assert int((~want[prune_ref.group_indices(segs, g)]).sum()) == k, (t, g)
        seen.append((t, targets))
    mask.event = event
    n_clipped = 0
    for it in range(8):
        res = dec.train_step(fm, im, caps, training=True, seed=70 + it)
        if clip:
            sync()
            g, w = dec.grads.to_numpy(), dec.params.to_numpy()
            live = prune_ref.unpack(mask.to_numpy(), mask.n_total)
        opt.step(dec.grads, 1e-2)
        sync()
        assert np.isfinite(float(res['loss']))
        dead = torch.from_numpy(~prune_ref.unpack(mask.to_numpy(), mask.n_total)).to(DEV)
        for buf in (dec.params, opt.m, opt.v, opt.ema):
            assert buf is None or not _bits(buf.flat[dead]).any(), it
        if clip:
            after = dec.grads.to_numpy()
            for k in g:
                off = dec.params.offsets[k]
                gk = np.where(live[off:off + g[k].size].reshape(g[k].shape), g[k], np.float32(0.0))
                ge = gk + np.float32(l2) * w[k]
                n_clipped += float(np.linalg.norm(ge.astype(np.float64))) > clip_norm
                assert_close(after[k] + np.float32(l2) * w[k], dr.clip_by_norm(ge, clip_norm), 1e-5, 'clipped gradient ' + k)
    assert [t for t, _ in seen] == [2, 4, 6, 8] and seen[-1][1] == [n // 2 for n in mask.group_sizes]
    assert dec.voided_steps() == 0 and (not clip or 0 < n_clipped < 8 * len(g))
    total_pruned = sum(mask.pruned_counts().values())
    assert total_pruned == sum(seen[-1][1])


# ---- 5. the CLIs ---------------------------------------------------------------------------------------------------------
def _run(name, argv):
    spec = importlib.util.spec_from_file_location('cli_%s_gpu_prune' % name, os.path.join(ROOT, 'src', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(argv)


def _no_error_files(logs):
    errs = glob.glob(os.path.join(logs, 'mscoco', 'error__*'))
    assert not errs, open(errs[0]).read()


def _step_of(path):
    return int(os.path.basename(path).split('-')[-1].split('.')[0])


def _newest(run_dir, prefix):
    return sorted(glob.glob(os.path.join(run_dir, prefix + '-*.npz')), key=_step_of)[-1]


def _zero_sets(path):
    """{variable: flat indices of its zeros} for the decoder's variables with two dimensions."""
    z = np.load(path)
    return {k: np.flatnonzero(z[k].reshape(-1) == 0) for k in z.files if k.startswith(ckpt.DEC_SCOPE) and z[k].ndim == 2}


def test_cli_prune_resume_keep_zeros_and_infer(tmp_path):
    """The tiny dataset and decoder-mode flags of test_gpu_ema.py: two epochs with events behind updates 2, 4, 6, 8 towards
    0.5; a resumed third epoch; cnn_finetune on top with --prune_keep_zeros; infer.py on the result."""
    from tests import tiny_dataset
    ds = tiny_dataset.make(str(tmp_path / 'mscoco'), n_train=16, n_valid=4, n_test=4)
    logs = str(tmp_path / 'experiments')
    common = ['--dataset_dir', ds, '--log_root', logs, '--cnn_name', 'inception_v3', '--cnn_fm_attention', 'Mixed_7c',
              '--cnn_input_size', '139,139', '--batch_size_eval', '4', '--rnn_size', '128', '--rnn_word_size', '64',
              '--batch_size_train', '8']
    pr = ['--prune_sparsity', '0.5', '--prune_start_step', '2', '--prune_end_step', '8', '--prune_every', '2']
    _run('train', common + pr + ['--train_mode', 'decoder', '--max_epoch', '2'])
    _no_error_files(logs)
    run_dir = os.path.join(logs, 'mscoco', 'radix_b256_add_LN_softmax_h8_tie_lstm_pr0.5_run_01')
    compact = _newest(run_dir, 'model_compact')
    steps = _step_of(compact)                                               # two epochs of this size save once, at the end
    assert steps >= 8 and steps % 2 == 0
    got = ckpt.sparsity(compact)
    assert len(got['variables']) >= 6
    for k, (nz, n) in got['variables'].items():
        assert n - nz == n // 2, k                                          # exactly floor(0.5 n) zeros
    # none forced elsewhere: the mask of model-N has as many clear bits as the prunable variables have zeros
    words = np.load(_newest(run_dir, 'model'))[prune.MASK_KEY]
    assert words.dtype == np.uint32
    clear = words.size * 32 - int(np.unpackbits(words.view(np.uint8)).sum())
    assert clear == sum(n // 2 for _, n in got['variables'].values())
    assert got['total'] - got['nonzero'] >= clear
    text = open(os.path.join(run_dir, 'model_size.txt')).read()
    assert 'Pruning ~ step %d ~ scheduled sparsity 0.500000' % steps in text and text.count('non-zero') == len(got['variables']) + 1
    zeros = _zero_sets(compact)
    # resumed: the mask is the one it had, bit for bit, and the zeros stay where they were
    _run('train', common + pr + ['--train_mode', 'decoder', '--max_epoch', '3'])
    _no_error_files(logs)
    full = _newest(run_dir, 'model')
    assert _step_of(full) == steps * 3 // 2 and np.array_equal(np.load(full)[prune.MASK_KEY], words)
    later = _zero_sets(_newest(run_dir, 'model_compact'))
    assert set(later) == set(zeros) and all(np.array_equal(later[k], zeros[k]) for k in zeros)
    before, after = np.load(compact), np.load(_newest(run_dir, 'model_compact'))
    k0 = sorted(zeros)[0]
    assert not np.array_equal(before[k0], after[k0])                        # (it trained on)
    # the next stage keeps the zeros: no schedule, no suffix of its own
    _run('train', common + ['--train_mode', 'cnn_finetune', '--name', 'lstm_pr0.5', '--prune_keep_zeros'])
    _no_error_files(logs)
    ft_dir = run_dir.replace('_run_01', '_cnnFT_run_01')
    ft = _zero_sets(_newest(ft_dir, 'model_compact'))
    assert set(ft) == set(zeros) and all(np.array_equal(ft[k], zeros[k]) for k in zeros)
    tuned = np.load(_newest(ft_dir, 'model_compact'))
    assert not np.array_equal(tuned[k0], after[k0])
    assert 'zeros of the loaded checkpoint kept' in open(os.path.join(ft_dir, 'model_size.txt')).read()
    _run('infer', ['--infer_checkpoints_dir', ft_dir, '--dataset_dir', ds, '--infer_set', 'test', '--batch_size_infer', '2',
                   '--get_metric_score', ''])
    import json
    caps = glob.glob(os.path.join(ft_dir, 'infer_test_beam_3_lpen_0.0', 'captions___*.json'))
    assert len(caps) == 1 and len(json.load(open(caps[0]))) == 4
