"""What the GPU tests of soft-target XE training (tests/test_gpu_soft_targets.py) rest on, checked without a GPU: the float64
restatement of the two rules (tests/soft_targets_ref.py) against the oracle and against its own derivative, the top-K
order, the input condition of the exact-id comparisons on the very operands the GPU tests build, and the interface:
SoftTargets, the command line's refusals and directory names, and header / binding / library agreeing on the entries."""
import ctypes as C
import importlib.util
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

import comic_amd._lib as L
from comic_amd import decoder as cdec, distill
from tests import exec_ops_ref as R
from tests import soft_targets_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------ reference identities ----------
@pytest.mark.parametrize('regime', [None, 'peaked'])
def test_reference_without_soft_targets_is_the_oracles_hard_loss(regime):
    c = S.xent_case(258, 8, regime)
    ref = S.soft_xent_ref(c['logits'], c['targets'], c['coef'], c['wmask'], c['lens'], 0.0, 0.0)
    lg, xent, dl, amax = R.xent_ref(c['logits'], c['targets'], c['coef'], c['wmask'], c['lens'])
    np.testing.assert_array_equal(ref['logits'], lg)
    np.testing.assert_allclose(ref['loss'], xent, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(ref['nll'], xent, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(ref['dlogits'], dl, rtol=1e-13, atol=1e-15)
    np.testing.assert_array_equal(ref['ids'], amax)


@pytest.mark.parametrize('eps,lam', S.SETTINGS)
def test_reference_gradient_rows_sum_to_zero_and_match_finite_differences(eps, lam):
    """d logits = d (sum_rows loss * coef / wmask) / d logits: a central difference of the reference loss, on live weighted
    rows; every live row of d logits sums to 0 and q sums to 1"""
    V, K = 258, 8
    c = S.xent_case(V, K)
    tab = (c['t_ids'][:S.T_ROWS], c['t_probs'][:S.T_ROWS])
    args = (c['targets'], c['coef'], c['wmask'], c['lens'], eps, lam) + tab
    z = c['logits'].astype(np.float64)
    ref = S.soft_xent_ref(z, *args)
    live = (np.arange(S.T_ROWS)[:, None] < c['lens'][None, :])
    assert np.abs(ref['q'].sum(-1) - 1.0)[live].max() < 1e-12
    assert np.abs(ref['dlogits'].sum(-1)).max() < 1e-15
    w, cf = c['wmask'][:, :S.T_ROWS].T.astype(np.float64), c['coef'][:, :S.T_ROWS].T.astype(np.float64)
    scale = np.divide(cf, w, out=np.zeros_like(cf), where=w > 0)

    def total(zz):
        return (S.soft_xent_ref(zz, *args)['loss'] * scale).sum()
    rng = np.random.default_rng(1)
    h = 1e-5
    for _ in range(40):
        t, b, v = rng.integers(S.T_ROWS), rng.integers(S.B), rng.integers(V)
        if rng.random() < 0.5:
            v = int(c['t_ids'][t, b, rng.integers(K)])                       # a column the teacher touches
        d = np.zeros_like(z)
        d[t, b, v] = h
        num = (total(z + d) - total(z - d)) / (2 * h)
        want = ref['dlogits'][t, b, v] if w[t, b] > 0 else 0.0
        # the difference quotient carries rounding noise of about 2^-52 * |total| / h = 2e-16 * 20 / 1e-5 = 4e-10 and a
        # truncation term of order h^2 = 1e-10 times a third derivative below 1: 2e-9 covers both
        assert abs(num - want) <= 1e-6 * abs(want) + 2e-9, (t, b, v, num, want)
    assert np.abs(ref['dlogits'][2, 1]).max() == 0                                  # the finished row


def test_reference_loss_is_the_cross_entropy_of_q():
    """lse(z) - (1 - eps - lam) z_y - eps mean(z) - lam sum_k q_T(ids_k) z_ids_k, the form the issue and the kernel use"""
    c = S.xent_case(258, 8)
    eps, lam = 0.1, 0.5
    ids, probs = c['t_ids'][:S.T_ROWS], c['t_probs'][:S.T_ROWS].astype(np.float64)
    ref = S.soft_xent_ref(c['logits'], c['targets'], c['coef'], c['wmask'], c['lens'], eps, lam, ids, probs)
    z = c['logits'].astype(np.float64)
    lse = np.log(np.exp(z - z.max(-1, keepdims=True)).sum(-1)) + z.max(-1)
    zy = np.take_along_axis(z, c['targets'][:, :S.T_ROWS].T[..., None].astype(np.int64), 2)[..., 0]
    with np.errstate(invalid='ignore'):                                         # (the finished row's table holds zeros)
        tz = (probs / probs.sum(-1, keepdims=True) * np.take_along_axis(z, ids.astype(np.int64), 2)).sum(-1)
    form = (lse - (1 - eps - lam) * zy - eps * z.mean(-1) - lam * tz) * c['wmask'][:, :S.T_ROWS].T
    live = np.arange(S.T_ROWS)[:, None] < c['lens'][None, :]
    np.testing.assert_allclose(ref['loss'][live], form[live], rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------ the top-K rule -----------------
def test_topk_rule_order_ties_and_extremes():
    p = np.array([[0.1, 0.3, 0.3, 0.05, 0.25], [0.2, 0.2, 0.2, 0.2, 0.2]])
    ids, val = S.topk_rule(p, 2)
    assert ids.tolist() == [[1, 2], [0, 1]] and val.tolist() == [[0.3, 0.3], [0.2, 0.2]]
    assert S.topk_rule(p, 3)[0].tolist() == [[1, 2, 4], [0, 1, 2]]            # the tie at the boundary: the lowest id
    assert S.topk_rule(p, 1)[0].tolist() == [[1], [0]]                        # K = 1
    ids, val = S.topk_rule(p, 5)                                              # K = V: a permutation, descending
    assert sorted(ids[0].tolist()) == [0, 1, 2, 3, 4] and (np.diff(val, axis=-1) <= 0).all()
    assert ids[0].tolist() == [1, 2, 4, 0, 3]


def test_teacher_reference_rows_without_a_token():
    z = S.teacher_logits(258, 3)
    ids, probs, pbar = S.teacher_topk_ref(z, S.WEIGHTS[3], S.LENS, S.T_ROWS, 2.0, 8)
    assert np.abs(pbar.sum(-1) - 1).max() < 1e-12
    dead = [(3, 0), (3, 1), (3, 2), (2, 1)]                                    # t >= T' and t >= lens[b]
    for t, b in dead:
        assert ids[t, b].tolist() == list(range(8)) and (probs[t, b] == 0).all()
    assert (probs[0] > 0).all() and (np.diff(probs[0], axis=-1) <= 0).all()
    assert all(len(set(r)) == 8 for r in ids.reshape(-1, 8).tolist())
    q = S.teacher_q(ids, probs, 258)
    assert np.abs(q[0].sum(-1) - 1).max() < 1e-12 and (q[3] == 0).all()


# ------------------------------------------------------------------------------------ the input condition ------------
@pytest.mark.parametrize('V,K,n,tau', S.TEACHER_CASES)
def test_gpu_operands_keep_their_ranks_apart(V, K, n, tau):
    """the reference's relative gap between consecutive ranks 1 .. K+1 exceeds 1e-5 on EVERY row of the operands the GPU
    test builds: no row is excused from the exact-id comparison.  (A failure here asks for other seeds, not for a skip.)"""
    z = S.teacher_logits(V, n)
    _, _, pbar = S.teacher_topk_ref(z, S.WEIGHTS[n], S.LENS, S.T_ROWS, tau, K)
    gaps = S.rank_gaps(pbar, K)
    print('  V=%d K=%d n=%d tau=%g: smallest gap %.3e' % (V, K, n, tau, gaps.min()))
    assert gaps.shape == (S.T_STRIDE, S.B) and gaps.min() > S.GAP_MIN


def test_gap_condition_holds_at_the_word_vocabulary_and_full_k():
    """further draws: V = 25 599 (the word baseline), K = 32 and K = 1, one to three members"""
    for V, K, n, tau in ((25599, 32, 3, 2.0), (25599, 1, 1, 1.0), (258, 32, 2, 1.0)):
        rng = np.random.default_rng(V + K)
        z = [(3 * rng.standard_normal((2, 2, V))).astype(np.float32) for _ in range(n)]
        pbar = S.mean_probability(z, [1.0 / n] * n, tau)
        assert S.rank_gaps(pbar, K).min() > S.GAP_MIN


@pytest.mark.parametrize('regime', [None, 'peaked'])
@pytest.mark.parametrize('K', S.K_CASES)
@pytest.mark.parametrize('V', S.V_CASES)
def test_xent_operands_cover_what_the_gpu_test_says(V, K, regime):
    c = S.xent_case(V, K, regime)
    live = np.arange(S.T_STRIDE)[:, None] < c['lens'][None, :]
    inside = (c['t_ids'] == c['targets'].T[..., None]).any(-1)
    assert inside[live].any() and (~inside[live]).any()                       # the target in the teacher's ids and outside
    assert all(len(set(r)) == K for r in c['t_ids'].reshape(-1, K).tolist()) and c['t_ids'].min() >= 0 and c['t_ids'].max() < V
    assert (c['t_probs'][live] > 0).all() and c['t_probs'].dtype == np.float32
    assert c['wmask'][2, 1] == 0 and c['lens'][1] < S.T_ROWS and V % 256 != 0


# ------------------------------------------------------------------------------------ the interface ------------------
def test_soft_targets_validation():
    s = cdec.SoftTargets()
    assert not s.active and (s.smoothing, s.teacher_weight, s.top_k, s.temperature) == (0.0, 0.0, 16, 1.0)
    assert cdec.SoftTargets(0.1).active and not cdec.SoftTargets(0.1).distils and cdec.SoftTargets(0.0, 0.5).distils
    assert cdec.SoftTargets(0.5, 0.5).active and cdec.SoftTargets(0.0, 1.0, 32, 4.0).top_k == 32
    for kw in (dict(smoothing=-0.1), dict(smoothing=1.0), dict(teacher_weight=-0.1), dict(teacher_weight=1.1),
               dict(smoothing=0.6, teacher_weight=0.5), dict(top_k=0), dict(top_k=33), dict(top_k=2.5), dict(temperature=0.0),
               dict(temperature=float('inf')), dict(temperature=float('nan')), dict(smoothing='0.1')):
        with pytest.raises(ValueError):
            cdec.SoftTargets(**kw)
    with pytest.raises(ValueError, match='exceeds the vocabulary'):
        cdec.SoftTargets(0.0, 0.5, 16).check_vocabulary(10)
    assert cdec.SoftTargets(0.1, 0.0, 16).ctx_key() == cdec.SoftTargets(0.1, 0.0, 8, 3.0).ctx_key()   # no table: K is not baked in
    assert cdec.SoftTargets(0.1, 0.5, 16).ctx_key() != cdec.SoftTargets(0.1, 0.5, 8).ctx_key()
    assert L.SOFT_MAX_K == 32


def test_soft_targets_from_config():
    from types import SimpleNamespace as NS
    assert cdec.soft_targets_from_config(NS()) is None
    assert cdec.soft_targets_from_config(NS(label_smoothing=0.0, distill_weight=0.5)) is None      # a weight without teachers
    s = cdec.soft_targets_from_config(NS(label_smoothing=0.1))
    assert (s.smoothing, s.teacher_weight) == (0.1, 0.0)
    s = cdec.soft_targets_from_config(NS(label_smoothing=0.1, distill_checkpoints='a,b', distill_weight=0.5, distill_top_k=8,
                                         distill_temperature=2.0))
    assert (s.smoothing, s.teacher_weight, s.top_k, s.temperature) == (0.1, 0.5, 8, 2.0)


def test_entries_are_declared_bound_and_exported():
    """include/comic_hip.h, _lib._SIGS and the cross-compiled library agree on the new entries, argument by argument, and the
    record's layout is the header's"""
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    decls = {name: [a.strip() for a in args.split(',')]
             for name, args in re.findall(r'\bint\s+(comic_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', header)}

    def ctype(a):
        if '*' in a:
            return L.P
        return {'int': C.c_int, 'float': C.c_float, 'int64_t': C.c_int64}[a.replace('const', '').split()[0]]
    names = ('comic_decoder_train_step_soft', 'comic_xent_soft', 'comic_teacher_topk')
    for name in names:
        res, args = L._SIGS[name]
        assert res is C.c_int and [ctype(a) for a in decls[name]] == list(args), name
    assert decls['comic_decoder_train_step_soft'][:-1] == decls['comic_decoder_train_step']       # the same arguments + the record
    assert decls['comic_decoder_train_step_soft'][-1] == 'const comic_soft_targets* soft'
    fields = re.search(r'typedef struct comic_soft_targets \{(.*?)\}', header, flags=re.S).group(1)
    assert [f.split()[-1].lstrip('*') for f in fields.split(';') if f.strip()] == [n for n, _ in L.SoftTargets._fields_]
    assert C.sizeof(L.SoftTargets) == 3 * 4 + 4 + 3 * 8
    assert int(re.search(r'#define COMIC_SOFT_MAX_K (\d+)', header).group(1)) == L.SOFT_MAX_K
    defined = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in defined.splitlines() if line.strip())
    assert set(names) <= exported, set(names) - exported


# ------------------------------------------------------------------------------------ the command line ---------------
def _train_module():
    spec = importlib.util.spec_from_file_location('cli_train_soft', os.path.join(ROOT, 'src', 'train.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _teacher(tmp_path, **changes):
    """a checkpoint path with a config.pkl beside it (the file itself is never opened by the checks)"""
    d = tmp_path / ('teacher_' + '_'.join(changes))                   # (no comma in the path: the flag splits on it)
    d.mkdir(exist_ok=True)
    cfg = dict(token_type='radix', radix_base=256, cnn_name='inception_v1', cnn_input_size=[224, 224], cnn_fm_attention='Mixed_4f')
    cfg.update(changes)
    with open(d / 'config.pkl', 'wb') as f:
        pickle.dump(cfg, f, 2)
    (d / 'model_compact-10.npz').write_bytes(b'')
    return str(d / 'model_compact-10.npz')


def test_cli_refusals_before_the_gpu(tmp_path):
    mod = _train_module()
    never = ['--log_root', '/nonexistent/never/created']
    good = _teacher(tmp_path)
    cases = [
        (['--train_mode', 'scst', '--label_smoothing', '0.1'], 'scst'),
        (['--train_mode', 'scst', '--distill_checkpoints', good, '--distill_weight', '0.5'], 'scst'),
        (['--train_mode', 'cnn_finetune', '--distill_checkpoints', good, '--distill_weight', '0.5'], 'train_mode decoder'),
        (['--label_smoothing', '1.0'], 'smoothing'),
        (['--label_smoothing', '-0.5'], 'smoothing'),
        (['--distill_weight', '0.5'], 'without --distill_checkpoints'),
        (['--distill_checkpoints', good], 'needs --distill_weight'),
        (['--distill_checkpoints', good, '--distill_weight', '1.5'], 'teacher_weight'),
        (['--distill_checkpoints', good, '--distill_weight', '0.95', '--label_smoothing', '0.1'], 'exceed'),
        (['--distill_checkpoints', good, '--distill_weight', '0.5', '--distill_top_k', '33'], 'top_k'),
        (['--distill_checkpoints', good, '--distill_weight', '0.5', '--distill_temperature', '0'], 'temperature'),
        (['--distill_checkpoints', good, '--distill_weight', '0.5', '--distill_weights', '0.5,0.5'], 'entries'),
        (['--distill_checkpoints', good + ',' + good, '--distill_weight', '0.5', '--distill_weights', '0.5,0.6'], 'sum to 1'),
        (['--distill_checkpoints', str(tmp_path / 'missing-1.npz'), '--distill_weight', '0.5'], 'not found'),
    ]
    for field, value in (('token_type', 'word'), ('radix_base', 128), ('cnn_name', 'inception_v3'), ('cnn_input_size', [299, 299]),
                         ('cnn_fm_attention', 'Mixed_5c')):
        cases.append((['--distill_checkpoints', _teacher(tmp_path, **{field: value}), '--distill_weight', '0.5'],
                      'differs from the student in %s' % field))
    for argv, word in cases:
        with pytest.raises(ValueError, match=word):
            mod.main(argv + never)
    assert not os.path.exists('/nonexistent/never/created')
    mod.refuse_bad_soft_options(vars(mod.create_parser().parse_args(['--distill_checkpoints', good, '--distill_weight', '0.5'])))
    mod.refuse_bad_soft_options(vars(mod.create_parser().parse_args(['--train_mode', 'cnn_finetune', '--label_smoothing', '0.1'])))


def test_teacher_vocabulary_size_is_checked_with_the_full_configuration(tmp_path):
    from types import SimpleNamespace as NS
    base = dict(token_type='word', radix_base=256, cnn_name='inception_v1', cnn_input_size=[224, 224], cnn_fm_attention='Mixed_4f')
    student = NS(itow={i: str(i) for i in range(30)}, **base)
    distill.check_teacher_config(student, NS(itow={i: str(i) for i in range(30)}, **base), 'p')
    with pytest.raises(ValueError, match='vocabulary size: 31 against 30'):
        distill.check_teacher_config(student, NS(itow={i: str(i) for i in range(31)}, **base), 'p')
    with pytest.raises(ValueError, match='no config.pkl'):
        distill.teacher_config(str(tmp_path / 'model_compact-1.npz'))


def test_cli_run_directories_and_configuration(tmp_path):
    mod = _train_module()
    good = _teacher(tmp_path)

    def build(*argv):
        args = mod.create_parser().parse_args(list(argv) + ['--log_root', str(tmp_path / 'exp'), '--dataset_dir', str(tmp_path)])
        kw, fn, _ = mod.build_kwargs(args)
        return os.path.basename(kw['log_path']), kw, fn
    plain, kw, fn = build()
    assert plain.endswith('_lstm_run_01') and '_kd' not in plain and fn == 'train_fn'
    assert not any(k.startswith('distill_') or k == 'label_smoothing' for k in kw)      # the configuration of always
    name, kw, _ = build('--label_smoothing', '0.1')
    assert name == plain.replace('_run_01', '_ls0.1_run_01') and kw['label_smoothing'] == 0.1
    assert not any(k.startswith('distill_') for k in kw)
    name, kw, _ = build('--distill_checkpoints', good, '--distill_weight', '0.5', '--distill_temperature', '2')
    assert name == plain.replace('_run_01', '_kd0.5_k16_t2_run_01')
    assert (kw['distill_weight'], kw['distill_top_k'], kw['distill_temperature'], kw['distill_checkpoints']) == (0.5, 16, 2.0, good)
    name, _, _ = build('--label_smoothing', '0.1', '--distill_checkpoints', good, '--distill_weight', '0.25', '--distill_top_k', '8')
    assert name == plain.replace('_run_01', '_ls0.1_kd0.25_k8_t1_run_01')
