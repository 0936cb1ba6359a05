"""Host side of constrained beam search, no GPU: BeamConstraints.check before anything touches the device, the translation
of a configuration's words into tokens, the infer.py flags and directory name, the new entries in the header and the
bindings, and the ban-rule reference of tests/beam_constraints_ref.py itself on hand-written histories."""
import ctypes as C
import importlib.util
import os
import re
from types import SimpleNamespace

import pytest

import comic_amd._lib as L
from comic_amd import decoder as cdec
from comic_amd.decoder import BeamConstraints
from comic_amd.ops import number_to_base
from tests.beam_constraints_ref import banned, ngram_bans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('comic_beam_bans', 'comic_beam_step_constrained', 'comic_decoder_beam_constrained_workspace',
               'comic_decoder_beam_constrained')
SPEC = cdec.DecoderSpec()            # radix-256: V = 258, end_id = 257


def test_defaults_are_inactive():
    assert not BeamConstraints().active
    assert BeamConstraints(min_length=1).active and BeamConstraints(no_repeat_ngram=1).active
    assert BeamConstraints(suppress=(3,)).active
    assert not BeamConstraints(ngram_stride=2).active          # a stride without an n-gram length bans nothing
    BeamConstraints().check(SPEC, 3, 14)
    assert BeamConstraints(2, 4, 2, [5, 6]) == BeamConstraints(2, 4, 2, (5, 6))
    assert len({BeamConstraints(2, 4, 2, [5, 6]), BeamConstraints(2, 4, 2, (5, 6)), BeamConstraints(2, 4, 2, (5,))}) == 2


@pytest.mark.parametrize('kw,field', [
    (dict(min_length=-1), 'min_length'),
    (dict(no_repeat_ngram=-2), 'no_repeat_ngram'),
    (dict(ngram_stride=0), 'ngram_stride'),
    (dict(no_repeat_ngram=3, ngram_stride=2), 'ngram_stride'),
    (dict(suppress=(SPEC.end_id,)), 'end_id'),
    (dict(suppress=(SPEC.V,)), 'suppress'),
    (dict(suppress=(-1,)), 'suppress'),
    (dict(suppress=tuple(range(33))), 'suppress'),
    (dict(min_length=14), 'min_length'),
])
def test_check_refuses(kw, field):
    with pytest.raises(ValueError, match=field):
        BeamConstraints(**kw).check(SPEC, 3, 14)


def test_check_refuses_a_vocabulary_too_small_for_the_beam():
    # V >= W + K + 1 + max_steps: 3 + 2 + 1 + 14 = 20
    BeamConstraints(min_length=2, suppress=(1, 2)).check(cdec.DecoderSpec(V=20, start_id=18, end_id=19), 3, 14)
    with pytest.raises(ValueError, match='V = 19'):
        BeamConstraints(min_length=2, suppress=(1, 2)).check(cdec.DecoderSpec(V=19, start_id=17, end_id=18), 3, 14)
    with pytest.raises(ValueError, match='V = 70000'):
        BeamConstraints(min_length=2).check(cdec.DecoderSpec(V=70000, start_id=1, end_id=2, token_type='word'), 3, 14)


def test_struct_matches_the_header():
    assert C.sizeof(L.BeamConstraints) == 4 * 4 + 32 * 4
    c = BeamConstraints(3, 4, 2, (9, 11)).c_struct()
    assert (c.min_length, c.no_repeat_ngram, c.ngram_stride, c.n_suppress) == (3, 4, 2, 2)
    assert list(c.suppress)[:3] == [9, 11, 0]
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    assert re.search(r'int32_t min_length, no_repeat_ngram, ngram_stride, n_suppress;\s*int32_t suppress\[32\];', header)


def _config(token_type, n_words=1000, **kw):
    wtoi = {'w%d' % k: k for k in range(n_words - 3)}
    wtoi.update({'<GO>': n_words - 3, '<EOS>': n_words - 2, '<UNK>': n_words - 1})
    return SimpleNamespace(token_type=token_type, wtoi=wtoi, radix_base=256, **kw)


def test_no_fields_no_constraints():
    assert cdec.constraints_from_config(_config('word')) is None
    assert cdec.constraints_from_config(_config('radix', infer_min_length=None, infer_suppress_words=None)) is None
    assert cdec.constraints_from_config(_config('word', infer_min_length=0, infer_no_repeat_ngram=0)) is None


def test_word_units():
    c = cdec.constraints_from_config(_config('word', infer_min_length=8, infer_no_repeat_ngram=3,
                                             infer_suppress_words='<UNK>,w5'))
    assert c == BeamConstraints(min_length=8, no_repeat_ngram=3, ngram_stride=1, suppress=(999, 5))
    with pytest.raises(ValueError, match='infer_suppress_words'):
        cdec.constraints_from_config(_config('word', infer_suppress_words=['nowhere']))


def test_radix_units():
    for n_words, word_len in ((1000, 2), (70000, 3)):
        assert len(number_to_base(n_words, 256)) == word_len
        c = cdec.constraints_from_config(_config('radix', n_words, infer_min_length=3, infer_no_repeat_ngram=1))
        assert c == BeamConstraints(min_length=3 * word_len, no_repeat_ngram=word_len, ngram_stride=word_len)
    with pytest.raises(ValueError, match='infer_suppress_words'):
        cdec.constraints_from_config(_config('radix', infer_suppress_words='w5'))


def test_char_units():
    c = cdec.constraints_from_config(_config('char', 60, infer_min_length=12, infer_no_repeat_ngram=4,
                                             infer_suppress_words=('w7',)))
    assert c == BeamConstraints(min_length=12, no_repeat_ngram=4, ngram_stride=1, suppress=(7,))


def _infer_cli():
    spec = importlib.util.spec_from_file_location('cli_infer_constraint_flags', os.path.join(ROOT, 'src', 'infer.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_infer_flags_are_absent_by_default_and_parsed_when_given():
    parser = _infer_cli().create_parser()
    overlay = {k: v for k, v in parser.parse_args([]).__dict__.items() if v is not None}
    for k in ('infer_min_length', 'infer_no_repeat_ngram', 'infer_suppress_words'):
        assert k not in overlay
    args = parser.parse_args(['--infer_min_length', '8', '--infer_no_repeat_ngram', '3', '--infer_suppress_words', '<UNK>,a',
                              '--infer_ensemble'])
    assert (args.infer_min_length, args.infer_no_repeat_ngram, args.infer_suppress_words) == (8, 3, '<UNK>,a')
    assert args.infer_ensemble is True


def test_directory_suffix():
    parser = _infer_cli().create_parser()
    assert cdec.constraints_dir_suffix(parser.parse_args([])) == ''
    assert cdec.constraints_dir_suffix(parser.parse_args(['--infer_min_length', '8'])) == '_min8_ngram0_sup0'
    assert cdec.constraints_dir_suffix(parser.parse_args(
        ['--infer_min_length', '3', '--infer_no_repeat_ngram', '2', '--infer_suppress_words', '<UNK>,a'])) == '_min3_ngram2_sup2'
    assert cdec.constraints_dir_suffix(SimpleNamespace(infer_no_repeat_ngram=1)) == '_min0_ngram1_sup0'


def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS
        m = re.search(r'\b%s\(' % name, header)
        assert m, name
        assert 'ops_rnn.py:49-112' in header[max(0, m.start() - 1500):m.start()], name
    assert 'typedef struct comic_beam_constraints' in header
    assert '#define COMIC_ABI_VERSION 1' in header               # additive change


# ---- the ban-rule reference itself ------------------------------------------------------------------------------------
def test_rule_unigrams():
    assert ngram_bans([], 1) == set()
    assert ngram_bans([4, 9, 4], 1) == {4, 9}
    # stride 1 by definition when n == 1 and s == 1; every emitted token is banned whatever its position


def test_rule_bigrams():
    assert ngram_bans([], 2) == set()                            # L = 0: L + 1 < n
    assert ngram_bans([5], 2) == set()                           # no complete window yet
    assert ngram_bans([5, 6, 5], 2) == {6}                       # "5 6" would repeat
    assert ngram_bans([5, 6, 7], 2) == set()
    assert ngram_bans([5, 6, 5, 7, 5], 2) == {6, 7}
    assert ngram_bans([5, 5], 2) == {5}                          # the window (0, 1) itself: "5 5" + 5


def test_rule_trigrams():
    assert ngram_bans([1], 3) == set()                           # L < n - 1
    assert ngram_bans([1, 2], 3) == set()                        # L = n - 1: a tail, but no window that ends before it
    assert ngram_bans([1, 2, 3, 1, 2], 3) == {3}
    assert ngram_bans([1, 2, 3, 2, 1], 3) == set()
    assert ngram_bans([1, 1, 1], 3) == {1}


def test_rule_stride_2():
    # words of two tokens, n = 2: the candidate completes a word only at odd L, and only aligned windows count
    assert ngram_bans([1, 2, 1], 2, 2) == {2}                    # word (1, 2) at position 0, tail 1 at an aligned start
    assert ngram_bans([1, 2, 1, 2], 2, 2) == set()               # L + 1 = 5: the candidate would start a word
    assert ngram_bans([9, 1, 2, 7, 1], 2, 2) == set()            # "1 2" occurs, but UNALIGNED (position 1): no ban
    assert ngram_bans([9, 1, 2, 7, 1], 2, 1) == {2}              # the same history under stride 1 bans it
    assert ngram_bans([1, 2, 3, 4, 1, 2, 3], 4, 2) == {4}
    assert ngram_bans([0, 1, 2, 3, 4, 5, 1, 2, 3], 4, 2) == set()    # L + 1 = 10, tail (1, 2, 3) only at the unaligned 1


def test_rule_min_length_and_suppress():
    assert banned([3, 4], 2, end_id=9, min_length=3) == {9}
    assert banned([3, 4, 5], 3, end_id=9, min_length=3) == set()
    assert banned([3, 4], 2, end_id=9, min_length=0, no_repeat_ngram=1, suppress=(7,)) == {3, 4, 7}
