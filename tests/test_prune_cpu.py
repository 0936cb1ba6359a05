"""`--prune_sparsity` on the host side (no GPU): the numpy reference of the selection against a brute-force loop, the
schedule, the targets, the CLI refusals, the configuration keys and directory names, and the mask's way through both
checkpoint containers."""
import importlib.util
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import comic_amd._lib as L
from comic_amd import checkpoint as ckpt, decoder as cdec, optim, prune
from tests import prune_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli(name):
    spec = importlib.util.spec_from_file_location('cli_%s_prune' % name, os.path.join(ROOT, 'src', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the reference of the selection --------------------------------------------------------------------------------------
def test_keys_order_by_magnitude_bits():
    w = np.array([-0.0, 0.0, 1e-42, -1e-42, 1.5, -1.5, 2.0 ** -126, np.inf], np.float32)
    k = prune_ref.keys(w)
    assert k[0] == k[1] == 0 and k[2] == k[3] and k[4] == k[5]
    assert k[1] < k[2] < k[6] < k[4] < k[7]                     # zero < denormal < smallest normal < 1.5 < inf


@pytest.mark.parametrize('seed', range(6))
def test_lexsort_reference_equals_brute_force_with_many_ties(seed):
    """Three magnitudes and their negatives over 3 groups with a gap between the segments: most elements tie, the index
    decides.  Two events: the second on the result of the first, one target below the pruned count (nothing may change)."""
    rng = np.random.default_rng(seed)
    segments = [(0, 17, 0), (64, 9, 1), (128, 30, 0), (192, 5, 2)]
    n = 256
    w = rng.choice(np.array([0.0, -0.0, 0.5, -0.5, 1e-40, 2.0], np.float32), n)
    live = np.ones(n, bool)
    for targets in ([11, 3, 0], [9, 9, 5], [47, 4, 5]):
        a = prune_ref.select(w, live, segments, targets)
        b = prune_ref.select_brute(w, live, segments, targets)
        assert np.array_equal(a, b), targets
        for g, k in enumerate(targets):
            idx = prune_ref.group_indices(segments, g)
            assert int((~a[idx]).sum()) == max(int((~live[idx]).sum()), min(k, idx.size))        # sticky, and exactly k
        assert np.array_equal(a | live, live)                                                      # nothing comes back
        outside = np.ones(n, bool)
        for f, c, _ in segments:
            outside[f:f + c] = False
        assert a[outside].all()                                                                    # padding stays live
        live = a


def test_reference_ties_go_by_lowest_index_and_pack_round_trip():
    w = np.array([1, -1, 1, 3, -1, 1], np.float32)
    live = prune_ref.select(w, np.ones(6, bool), [(0, 6, 0)], [3])
    assert live.tolist() == [False, False, False, True, True, True]
    words = prune_ref.pack(live)
    assert words.dtype == np.uint32 and words.tolist() == [0xFFFFFFF8]
    assert np.array_equal(prune_ref.unpack(words, 6), live)
    big = np.random.default_rng(0).random(1000) < 0.5
    assert np.array_equal(prune_ref.unpack(prune_ref.pack(big), 1000), big) and prune_ref.pack(big).size == 32


# ---- schedule and targets ------------------------------------------------------------------------------------------------
def test_schedule_by_hand():
    s_f, t0, t1 = 0.8, 100, 500
    f = optim.prune_sparsity_at
    assert f is prune.prune_sparsity_at
    assert f(t0, s_f, t0, t1) == 0.0 and f(t1, s_f, t0, t1) == 0.8
    # t = 200: (t - t0) / (t1 - t0) = 1/4; 1 - (3/4)^3 = 1 - 27/64 = 37/64 = 0.578125; 0.8 * 0.578125 = 0.4625
    assert f(200, s_f, t0, t1) == pytest.approx(0.4625, rel=1e-15)
    # t = 300: 1 - (1/2)^3 = 7/8; 0.8 * 7/8 = 0.7
    assert f(300, s_f, t0, t1) == pytest.approx(0.7, rel=1e-15)
    assert f(0, s_f, t0, t1) == 0.0 and f(99, s_f, t0, t1) == 0.0
    assert f(501, s_f, t0, t1) == 0.8 and f(10 ** 9, s_f, t0, t1) == 0.8
    steps = [f(t, s_f, t0, t1) for t in range(0, 700)]
    assert all(b >= a for a, b in zip(steps, steps[1:]))
    assert [t for t in range(0, 700) if prune.is_event(t, t0, t1, 100)] == [100, 200, 300, 400, 500]


def test_targets_are_floored_in_float64():
    # sizes where the float32 product rounds across the integer: (s, n, floor of the float64 product)
    for s, n, want in ((0.7, 5700000, 3989999), (0.9, 16777217, 15099495)):
        assert prune.target_count(s, n) == want == math.floor(Fraction(s) * n)
        assert int(math.floor(np.float32(s) * np.float32(n))) != want
    assert prune.target_count(0.5, 1) == 0 and prune.target_count(0.5, 3) == 1 and prune.target_count(0.0, 7) == 0
    assert prune.target_count(0.4625, 100003) == 46251


def test_groups_count_real_elements_not_padding():
    spec = cdec.DecoderSpec(D=16, E=8, V=20, C=12, Cg=12, H=2, M=4)
    shapes = spec.param_shapes()
    offsets, off = {}, 0
    for k, shp in shapes.items():
        offsets[k] = off
        off += (int(np.prod(shp)) if len(shp) else 1 + 63) // 64 * 64 + 64
    seg = prune.segments_of(shapes, offsets, None, 'layer')
    assert [s[0] for s in seg] == [k for k in shapes if k in prune.PRUNABLE] and len(seg) >= 6
    assert all(len(shapes[s[0]]) == 2 and s[2] == int(np.prod(shapes[s[0]])) for s in seg)
    assert [s[3] for s in seg] == list(range(len(seg)))
    assert not [k for k in shapes if len(shapes[k]) == 2 and k not in prune.PRUNABLE]           # every matrix is prunable
    assert {s[3] for s in prune.segments_of(shapes, offsets, None, 'global')} == {0}
    two = prune.segments_of(shapes, offsets, ('W_o', 'K'), 'layer')
    assert [s[0] for s in two] == sorted(('W_o', 'K'), key=lambda k: offsets[k])
    with pytest.raises(ValueError, match='no variable'):
        prune.segments_of({k: v for k, v in shapes.items() if k != 'K'}, offsets, ('K',), 'layer')


# ---- flags ---------------------------------------------------------------------------------------------------------------
BAD = [(['--prune_sparsity', '1.0'], 'prune_sparsity'), (['--prune_sparsity', '-0.1'], 'prune_sparsity'),
       (['--prune_sparsity', 'nan'], 'prune_sparsity'),
       (['--prune_sparsity', '0.5', '--prune_keep_zeros'], 'prune_keep_zeros'),
       (['--prune_sparsity', '0.5', '--prune_variables', 'W_m,nope'], 'unknown variable'),
       (['--prune_sparsity', '0.5', '--prune_variables', 'b'], 'never pruned'),
       (['--prune_sparsity', '0.5', '--prune_variables', 'tau'], 'never pruned'),
       (['--prune_sparsity', '0.5', '--prune_variables', 'ln_g'], 'never pruned'),
       (['--prune_keep_zeros', '--prune_variables', 'b_o'], 'never pruned'),
       (['--prune_sparsity', '0.5', '--prune_variables', 'K,K'], 'twice'),
       (['--prune_sparsity', '0.5', '--prune_every', '0'], 'prune_every'),
       (['--prune_sparsity', '0.5', '--prune_start_step', '-5'], 'prune_start_step'),
       (['--prune_sparsity', '0.5', '--prune_start_step', '100', '--prune_end_step', '100'], 'prune_end_step'),
       (['--prune_sparsity', '0.5', '--prune_start_step', '100', '--prune_end_step', '50'], 'prune_end_step'),
       (['--prune_sparsity', '0.5', '--prune_start_step', '100', '--prune_end_step', '350'], 'multiple'),
       (['--prune_start_step', '100'], 'without --prune_sparsity'), (['--prune_scope', 'global'], 'without --prune_sparsity'),
       (['--prune_variables', 'K'], 'without --prune_sparsity'), (['--prune_every', '10'], 'without --prune_sparsity')]


@pytest.mark.parametrize('argv,match', BAD, ids=[' '.join(a) for a, _ in BAD])
def test_train_refuses_bad_prune_flags_before_the_gpu(argv, match):
    mod = _cli('train')
    with pytest.raises(ValueError, match=match):
        # main() refuses right after parsing: nothing is imported from torch, no directory is created
        mod.main(argv + ['--log_root', '/nonexistent/never/created'])
    kw = vars(mod.create_parser().parse_args(argv))
    with pytest.raises(ValueError, match=match):
        mod.check_supported(dict(kw, train_mode='decoder', cnn_dtype='bf16'))
    assert not os.path.exists('/nonexistent/never/created')


def test_default_flags_leave_no_key_and_suffixes(tmp_path):
    mod = _cli('train')
    root = ['--log_root', str(tmp_path)]
    mod.check_supported({'train_mode': 'decoder', 'cnn_dtype': 'bf16'})             # (a configuration from before the flags)
    plain, _, _ = mod.build_kwargs(mod.create_parser().parse_args(root))
    assert not [k for k in plain if k.startswith('prune')]
    zero, _, _ = mod.build_kwargs(mod.create_parser().parse_args(root + ['--prune_sparsity', '0']))
    assert zero == plain
    assert os.path.basename(plain['log_path']) == 'radix_b256_add_LN_softmax_h8_tie_lstm_run_01'
    on, _, _ = mod.build_kwargs(mod.create_parser().parse_args(root + ['--prune_sparsity', '0.8']))
    assert os.path.basename(on['log_path']) == 'radix_b256_add_LN_softmax_h8_tie_lstm_pr0.8_run_01'
    assert {k: on[k] for k in prune.FLAGS} == dict(prune.DEFAULTS, prune_sparsity=0.8)
    for k in prune.FLAGS + ('log_path', 'save_path'):
        on.pop(k)
        plain.pop(k, None)
    assert on == plain
    glob_, _, _ = mod.build_kwargs(mod.create_parser().parse_args(root + ['--prune_sparsity', '0.8', '--prune_scope', 'global',
                                                                          '--label_smoothing', '0.1']))
    assert os.path.basename(glob_['log_path']) == 'radix_b256_add_LN_softmax_h8_tie_lstm_pr0.8g_ls0.1_run_01'
    # --prune_keep_zeros adds no suffix: the stage is named after its checkpoint (`--name lstm_pr0.8` continues the run above)
    os.makedirs(tmp_path / 'mscoco' / 'radix_b256_add_LN_softmax_h8_tie_lstm_pr0.8_run_01')
    keep, _, _ = mod.build_kwargs(mod.create_parser().parse_args(root + ['--prune_keep_zeros', '--name', 'lstm_pr0.8',
                                                                         '--train_mode', 'cnn_finetune']))
    assert os.path.basename(keep['log_path']) == 'radix_b256_add_LN_softmax_h8_tie_lstm_pr0.8_cnnFT_run_01'
    assert keep['checkpoint_path'].endswith('radix_b256_add_LN_softmax_h8_tie_lstm_pr0.8_run_01')
    assert keep['prune_keep_zeros'] is True and keep['prune_sparsity'] == 0.0


def test_schedule_defaults_from_max_step():
    from types import SimpleNamespace as NS
    assert optim.PruneSpec.from_config(NS(), 1000) is None
    assert optim.PruneSpec.from_config(NS(prune_sparsity=0.0, prune_keep_zeros=False), 1000) is None
    s = optim.PruneSpec.from_config(NS(prune_sparsity=0.5), 1000)                   # 100 ... 600 every 100
    assert (s.start, s.end, s.every, s.scope, s.variables, s.keep_zeros) == (100, 600, 100, 'layer', None, False)
    s = optim.PruneSpec.from_config(NS(prune_sparsity=0.5, prune_every=70), 1000)   # 600 moved down: 100 + 7 * 70
    assert (s.start, s.end) == (100, 590) and s.event_at(590) and not s.event_at(600) and s.event_at(100)
    assert s.sparsity_at(590) == 0.5 and s.sparsity_at(99) == 0.0
    s = optim.PruneSpec.from_config(NS(prune_sparsity=0.5, prune_start_step=0, prune_end_step=6, prune_every=2,
                                       prune_scope='global', prune_variables='K,W_o'), 1000)
    assert (s.start, s.end, s.every, s.scope, s.variables) == (0, 6, 2, 'global', ('K', 'W_o'))
    with pytest.raises(ValueError, match='prune_end_step'):
        optim.PruneSpec.from_config(NS(prune_sparsity=0.5), 100)                    # no event fits between 10 and 60
    k = optim.PruneSpec.from_config(NS(prune_keep_zeros=True), 1000)
    assert k.keep_zeros and not k.event_at(100) and k.variables is None


# ---- the ABI and the containers ------------------------------------------------------------------------------------------
def test_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    for name in ('comic_prune_workspace_bytes', 'comic_prune_select', 'comic_prune_mask_buffer', 'comic_prune_mask_from_zeros',
                 'comic_adam_tf_masked', 'comic_momentum_tf_masked'):
        assert re.search(r'\b%s\(' % name, header), name
        assert name in L.EXPORTED_SYMBOLS
    assert '#define COMIC_ABI_VERSION 1' in header               # additive change
    src = open(os.path.join(os.path.dirname(prune.__file__), 'csrc', 'Makefile')).read()
    assert ' prune.hip ' in src


@pytest.mark.parametrize('fmt', ['npz', 'tf'])
def test_mask_travels_through_the_full_checkpoint(tmp_path, fmt):
    spec = cdec.DecoderSpec(D=16, E=8, V=20, C=12, Cg=12, H=2, M=4)
    rng = np.random.default_rng(2)
    dec = {k: rng.standard_normal(v).astype(np.float32) for k, v in spec.param_shapes().items()}
    cnn = {'InceptionV3/Conv2d_1a_3x3/weights': rng.standard_normal((3, 3, 3, 4)).astype(np.float32)}
    words = rng.integers(0, 2 ** 32, 37, dtype=np.uint64).astype(np.uint32)
    words[0], words[1] = 0xFFFFFFFF, 0x80000000
    path = ckpt.save(str(tmp_path / 'model'), 5, cnn, spec, dec, {prune.MASK_KEY: words}, fmt=fmt)
    _, d2, got = ckpt.restore(path, list(cnn), spec, resume_training=True)
    assert got[prune.MASK_KEY].dtype == np.uint32 and np.array_equal(got[prune.MASK_KEY], words)
    assert all(np.array_equal(d2[k], dec[k]) for k in dec)
    _, _, none = ckpt.restore(path, list(cnn), spec, resume_training=False)
    assert none == {}                                            # a new stage does not inherit the mask: it keeps zeros


def test_sparsity_of_a_compact_checkpoint_and_the_size_block(tmp_path):
    spec = cdec.DecoderSpec(D=16, E=8, V=20, C=12, Cg=12, H=2, M=4)
    rng = np.random.default_rng(4)
    dec = {k: (1 + rng.random(v)).astype(np.float32) for k, v in spec.param_shapes().items()}
    dec['W_o'].reshape(-1)[:10] = 0.0
    dec['K'].reshape(-1)[::2] = 0.0
    path = ckpt.save(str(tmp_path / 'model_compact'), 7, {}, spec, dec)
    names = ckpt.decoder_var_names(spec)
    for got in (ckpt.sparsity(path, spec), ckpt.sparsity(path)):
        assert set(got['variables']) == {names[k] for k in dec if k in prune.PRUNABLE}
        assert got['variables'][names['W_o']] == (dec['W_o'].size - 10, dec['W_o'].size)
        assert got['variables'][names['K']] == (dec['K'].size - (dec['K'].size + 1) // 2, dec['K'].size)
        total = sum(v.size for v in dec.values())
        assert got['total'] == total and got['nonzero'] == total - 10 - (dec['K'].size + 1) // 2
    block = prune.size_block(7, 0.4625, {'K': (3, 8)}, 11, 20)
    assert 'step 7' in block and '0.462500' in block and 'K : 3 / 8 non-zero' in block and '11 / 20 non-zero' in block
