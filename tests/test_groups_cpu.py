"""Host side of diverse beam search, no GPU: BeamGroups.check before anything touches the device, the struct, the new
entries in the header and the bindings, the infer.py flags and directory name, and the grouped-step reference of
tests/beam_groups_ref.py itself on tiny hand-made inputs."""
import ctypes as C
import importlib.util
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import comic_amd._lib as L
from comic_amd import decoder as cdec
from comic_amd.decoder import BeamGroups
from tests.beam_groups_ref import init_state, ref_select_groups
from tests.test_gpu_ensemble import ref_select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('comic_beam_step_diverse', 'comic_decoder_beam_diverse_workspace', 'comic_decoder_beam_diverse')


def test_defaults_are_inactive():
    assert not BeamGroups().active and BeamGroups().key() == (1, 0.0)
    assert not BeamGroups(1, 0.5).active                       # one group is the plain beam whatever the diversity
    assert BeamGroups(2).active and BeamGroups(3, 0.5).active
    BeamGroups().check(3)
    BeamGroups(3, 0.5).check(6, 258)
    assert BeamGroups(3, 0.5) == BeamGroups(3.0, '0.5') and BeamGroups(3, 0.5) != BeamGroups(3, 0.25)
    assert len({BeamGroups(3, 0.5), BeamGroups(3, 0.5), BeamGroups(2, 0.5)}) == 2
    assert repr(BeamGroups(3, 0.5)) == 'BeamGroups(groups=3, diversity=0.5)'


@pytest.mark.parametrize('kw,beam,field', [
    (dict(groups=0), 6, 'groups must be'),
    (dict(groups=-2), 6, 'groups must be'),
    (dict(groups=7), 6, 'groups 7 exceeds'),
    (dict(groups=4), 6, 'groups 4 does not divide'),
    (dict(groups=2, diversity=-0.1), 6, 'diversity'),
    (dict(groups=2, diversity=float('nan')), 6, 'diversity'),
    (dict(groups=2, diversity=float('inf')), 6, 'diversity'),
])
def test_check_refuses(kw, beam, field):
    with pytest.raises(ValueError, match=field):
        BeamGroups(**kw).check(beam, 258)


def test_check_refuses_a_group_wider_than_the_vocabulary():
    BeamGroups(2, 0.5).check(8, 4)
    with pytest.raises(ValueError, match='groups'):
        BeamGroups(2, 0.5).check(8, 3)


def test_struct_matches_the_header():
    assert C.sizeof(L.BeamGroups) == 8
    g = BeamGroups(3, 0.5).c_struct()
    assert (g.groups, g.diversity) == (3, 0.5)
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    assert re.search(r'typedef struct comic_beam_groups \{\s*int32_t groups;\s*float diversity;\s*\} comic_beam_groups;', header)


def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS
        m = re.search(r'\b%s\(' % name, header)
        assert m, name
        assert 'ops_rnn.py:49-112' in header[max(0, m.start() - 1500):m.start()], name
    assert '#define COMIC_ABI_VERSION 1' in header               # additive change


def _infer_cli():
    spec = importlib.util.spec_from_file_location('cli_infer_group_flags', os.path.join(ROOT, 'src', 'infer.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_infer_flags_are_absent_by_default_and_parsed_when_given():
    parser = _infer_cli().create_parser()
    overlay = {k: v for k, v in parser.parse_args([]).__dict__.items() if v is not None}
    assert 'infer_beam_groups' not in overlay and 'infer_diversity' not in overlay
    args = parser.parse_args(['--infer_beam_groups', '3', '--infer_diversity', '0.5', '--infer_beam_size', '6',
                              '--infer_ensemble', '--infer_min_length', '4'])
    assert (args.infer_beam_groups, args.infer_diversity, args.infer_beam_size) == (3, 0.5, 6)
    assert args.infer_ensemble is True and args.infer_min_length == 4


def test_groups_from_config():
    assert cdec.groups_from_config(SimpleNamespace(infer_beam_size=6)) is None
    assert cdec.groups_from_config(SimpleNamespace(infer_beam_size=6, infer_beam_groups=None, infer_diversity=None)) is None
    assert cdec.groups_from_config(SimpleNamespace(infer_beam_size=6, infer_beam_groups=3, infer_diversity=0.5)) \
        == BeamGroups(3, 0.5)
    assert cdec.groups_from_config(SimpleNamespace(infer_beam_size=6, infer_beam_groups=2)) == BeamGroups(2, 0.0)
    assert not cdec.groups_from_config(SimpleNamespace(infer_beam_size=6, infer_diversity=0.5)).active
    with pytest.raises(ValueError, match='groups 4 does not divide'):
        cdec.groups_from_config(SimpleNamespace(infer_beam_size=6, infer_beam_groups=4))


def test_directory_suffix():
    parser = _infer_cli().create_parser()
    assert cdec.groups_dir_suffix(parser.parse_args([])) == ''
    assert cdec.groups_dir_suffix(parser.parse_args(['--infer_beam_groups', '3', '--infer_diversity', '0.5'])) == '_grp3_div0.5'
    assert cdec.groups_dir_suffix(parser.parse_args(['--infer_beam_groups', '2'])) == '_grp2_div0'
    assert cdec.groups_dir_suffix(SimpleNamespace(infer_beam_groups=6, infer_diversity=1.0)) == '_grp6_div1'
    both = parser.parse_args(['--infer_min_length', '8', '--infer_beam_groups', '3', '--infer_diversity', '0.25'])
    assert cdec.constraints_dir_suffix(both) + cdec.groups_dir_suffix(both) == '_min8_ngram0_sup0_grp3_div0.25'


def test_final_log_probs_adds_the_penalty_back():
    """Two groups of one slot, both emit token 4 at the last step: group 1's rank is its total minus 0.5; an <EOS> is
    never penalised."""
    grp = BeamGroups(2, 0.5)
    scores = np.array([[[-1.0, -2.5]], [[-3.0, -4.5]]], np.float32)            # [T=2, B=1, W=2]
    np.testing.assert_array_equal(grp.final_log_probs(scores, np.array([[[1, 1]], [[4, 4]]]), np.array([[2, 2]]), 9),
                                  np.array([[-3.0, -4.0]], np.float32))
    np.testing.assert_array_equal(grp.final_log_probs(scores, np.array([[[1, 1]], [[9, 9]]]), np.array([[2, 2]]), 9),
                                  np.array([[-3.0, -4.5]], np.float32))


# ---- the grouped-step reference itself ----------------------------------------------------------------------------------
END = 4


def _lp(rows):
    """[B=1, W, V=5] log-probabilities from rows of probabilities."""
    return np.log(np.asarray(rows, np.float64))[None]


def _mid(W):
    return np.zeros((1, W), np.float32), np.zeros((1, W), np.int32), np.full((1, W), 2, np.int64)


# every beam prefers token 1, then 2, then 0, then 3
ROW = [0.15, 0.4, 0.3, 0.1, 0.05]
ROW_B = [0.16, 0.38, 0.31, 0.1, 0.05]


def test_ref_one_group_is_ref_select():
    rng = np.random.default_rng(0)
    lp = np.log(rng.dirichlet(np.ones(7), (2, 4)))
    log_probs = -rng.uniform(1, 6, (2, 4))
    finished = np.array([[0, 1, 0, 0], [0, 0, 0, 1]], np.int32)
    lengths = rng.integers(1, 7, (2, 4)).astype(np.int64)
    for lpw in (0.0, 0.7):
        a = ref_select_groups(lp, log_probs, finished, lengths, 6, lpw, 1, 0.5)
        b = ref_select(lp, log_probs, finished, lengths, 6, lpw)
        assert sorted(a) == sorted(b)
        for k in b:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_ref_zero_diversity_makes_all_groups_equal():
    lp = _lp([ROW, ROW_B] * 3)                                  # three groups of two beams, the same rows
    r = ref_select_groups(lp, *_mid(6), END, 0.0, 3, 0.0)
    for g in (1, 2):
        np.testing.assert_array_equal(r['word'][:, 2 * g:2 * g + 2], r['word'][:, :2])
        np.testing.assert_array_equal(r['parent'][:, 2 * g:2 * g + 2], r['parent'][:, :2] + 2 * g)
        np.testing.assert_array_equal(r['scores'][:, 2 * g:2 * g + 2], r['scores'][:, :2])
    np.testing.assert_array_equal(r['word'][0, :2], [1, 1])      # tokens 1 of both beams: 0.4 and 0.38


def test_ref_group_0_is_ref_select_at_its_width():
    lp = _lp([ROW, ROW_B] * 3)
    r = ref_select_groups(lp, *_mid(6), END, 0.0, 3, 2.0)
    lp0, fin0, len0 = _mid(2)
    n = ref_select(lp[:, :2], lp0, fin0, len0, END, 0.0)
    for k in ('word', 'parent', 'scores', 'log_probs', 'finished', 'lengths'):
        np.testing.assert_array_equal(r[k][:, :2], n[k], err_msg=k)


def test_ref_penalty_pushes_later_groups_off_the_words_of_earlier_ones():
    lp = _lp([ROW] * 3)                                         # three groups of one beam
    r = ref_select_groups(lp, *_mid(3), END, 0.0, 3, 1.0)
    # group 0 takes 1; group 1 sees log .4 - 1 < log .3 and takes 2; group 2 sees 1 and 2 penalised once each and takes 0
    np.testing.assert_array_equal(r['word'], [[1, 2, 0]])
    np.testing.assert_array_equal(r['parent'], [[0, 1, 2]])
    np.testing.assert_allclose(r['scores'], np.log([[0.4, 0.3, 0.15]]))
    # counts add up: with a small penalty group 1 stays on 1, and group 2 pays it TWICE for token 1
    r = ref_select_groups(lp, *_mid(3), END, 0.0, 3, 0.2)
    np.testing.assert_array_equal(r['word'], [[1, 1, 2]])       # group 2: log .4 - .4 = -1.316 < log .3 = -1.204
    np.testing.assert_allclose(r['scores'], [[np.log(0.4), np.log(0.4) - np.float32(0.2), np.log(0.3)]])


def test_ref_eos_is_never_penalised():
    row = [0.1, 0.1, 0.1, 0.1, 0.6]                             # <EOS> is the best token of every beam
    r = ref_select_groups(_lp([row] * 3), *_mid(3), END, 0.0, 3, 5.0)
    np.testing.assert_array_equal(r['word'], [[END, END, END]])
    np.testing.assert_allclose(r['scores'], np.log([[0.6, 0.6, 0.6]]))
    np.testing.assert_array_equal(r['finished'], [[1, 1, 1]])


def test_ref_a_finished_beam_is_never_penalised():
    """Group 1's only beam is finished: its candidates are _mask_probs' (0 at <EOS>), whatever group 0 chose -- and a
    finished beam of an EARLIER group counts with its <EOS>, which nobody pays for."""
    log_probs, finished, lengths = _mid(2)
    finished[0, 1] = 1
    log_probs[0, 1] = -3.0
    r = ref_select_groups(_lp([ROW] * 2), log_probs, finished, lengths, END, 0.0, 2, 5.0)
    np.testing.assert_array_equal(r['word'], [[1, END]])
    np.testing.assert_allclose(r['scores'], [[np.log(0.4), -3.0]])
    np.testing.assert_array_equal(r['lengths'], [[3, 2]])


def test_ref_state_carries_the_unpenalised_total():
    lp = _lp([ROW] * 2)
    log_probs, finished, lengths = _mid(2)
    log_probs[:] = [[-1.0, -2.0]]
    r = ref_select_groups(lp, log_probs, finished, lengths, END, 0.0, 2, 0.1)
    np.testing.assert_array_equal(r['word'], [[1, 1]])
    np.testing.assert_allclose(r['scores'], [[-1.0 + np.log(0.4), -2.0 + np.log(0.4) - np.float32(0.1)]])
    np.testing.assert_allclose(r['log_probs'], [[-1.0 + np.log(0.4), -2.0 + np.log(0.4)]])
    # with a length penalty the rank is score - penalty, the state still the total
    r = ref_select_groups(lp, log_probs, finished, lengths, END, 0.7, 2, 0.1)
    div = ((5.0 + 3) / 6.0) ** np.float64(np.float32(0.7))
    np.testing.assert_allclose(r['scores'], [[(-1.0 + np.log(0.4)) / div, (-2.0 + np.log(0.4)) / div - np.float32(0.1)]])
    np.testing.assert_allclose(r['log_probs'], [[-1.0 + np.log(0.4), -2.0 + np.log(0.4)]])


def test_ref_initial_state():
    log_probs, finished, lengths = init_state(2, 6, 3)
    np.testing.assert_array_equal(finished, [[0, 1, 0, 1, 0, 1]] * 2)
    assert (log_probs[:, ::2] == 0).all() and np.isneginf(log_probs[:, 1::2]).all() and (lengths == 0).all()
    r = ref_select_groups(_lp([ROW] * 6).repeat(2, axis=0), log_probs, finished, lengths, END, 0.0, 3, 1.0)
    np.testing.assert_array_equal(r['parent'], [[0, 0, 2, 2, 4, 4]] * 2)       # every slot descends from its group's first
    # group 0: 1, 2.  group 1: 0 (-1.897) and 1 (log .4 - 1 = -1.916) beat 2 (-2.204) and 3 (-2.303).  group 2: token 1 is
    # penalised twice, 0 and 2 once: 2 (-2.204), 3 (-2.303)
    np.testing.assert_array_equal(r['word'], [[1, 2, 0, 1, 2, 3]] * 2)
