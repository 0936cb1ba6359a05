"""Forced-prefix decoding on the host (no GPU compute): decoder.BeamPrefix and its checks, BeamOptions(prefix=), the
comic_beam_prefix record and its three entries in the header and the library, the prefixed workspace query against the
unprefixed one, the executor's refusals with null descs, the numpy rule of tests/beam_prefix_ref.py on hand-made rows, and
the configuration / command line: encodings, words outside the vocabulary, the directory suffix."""
import ctypes as C
import importlib.util
import itertools
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import comic_amd._lib as L
from comic_amd import decoder as cdec
from comic_amd.decoder import (BeamConstraints, BeamGroups, BeamOptions, BeamPrefix, BeamRequired, BeamSampling,
                               BeamTruncation)
from tests import beam_prefix_ref as pref
from tests.beam_constraints_ref import pack_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'beam_workspace_sizes.json')))
NEW_SYMBOLS = ('comic_beam_prefix_mask', 'comic_decoder_beam_search_prefixed_workspace', 'comic_decoder_beam_search_prefixed')
SPEC = SimpleNamespace(V=258, end_id=257, start_id=256)
PFX = BeamPrefix(np.array([[7, 9, -1], [11, -1, -1]], np.int32))


# ---- decoder.BeamPrefix ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ids,spec,batch,max_steps,what', [
    (np.zeros(3, np.int32), SPEC, None, 10, r'ids must be \[B, max_tokens\]'),
    (np.zeros((2, 1, 1), np.int32), SPEC, None, 10, r'ids must be \[B, max_tokens\]'),
    (np.zeros((3, 2), np.int32), SPEC, 2, 10, 'the table holds 3 images, the batch 2'),
    (np.zeros((2, 0), np.int32), SPEC, 2, 10, r'max_tokens 0 is outside \[1,10\)'),
    (np.zeros((2, 10), np.int32), SPEC, 2, 10, r'max_tokens 10 is outside \[1,10\)'),
    (np.array([[3, -1, 4], [1, 2, 3]], np.int32), SPEC, 2, 10, 'a -1 is followed by a token'),
    (np.array([[3, 258]], np.int32), SPEC, 1, 10, 'token 258 is outside the vocabulary of 258'),
    (np.array([[3, 257]], np.int32), SPEC, 1, 10, 'end_id 257 cannot be part of a prefix'),
    (np.array([[256, 3]], np.int32), SPEC, 1, 10, 'start_id 256 cannot be part of a prefix'),
    (np.array([[3]], np.int32), SimpleNamespace(V=65537, end_id=1, start_id=0), 1, 10, 'V = 65537 exceeds 65536'),
])
def test_check_refuses(ids, spec, batch, max_steps, what):
    with pytest.raises(ValueError, match=what):
        BeamPrefix(ids).check(spec, 3, batch, max_steps)


def test_check_passes_ragged_rows_and_the_largest_vocabulary():
    PFX.check(SPEC, 3, 2, 4)
    BeamPrefix(np.full((2, 3), -1, np.int32)).check(SPEC, 3, 2, 10)              # nobody has a prefix
    BeamPrefix(np.array([[65535]], np.int32)).check(SimpleNamespace(V=65536, end_id=1, start_id=0), 1, 1, 3)
    assert PFX.lengths.tolist() == [2, 1] and PFX.max_tokens == 3 and PFX.active
    assert BeamPrefix(np.array([[1, 2], [-1, -1]], np.int32)).lengths.tolist() == [2, 0]
    assert PFX.c_struct().max_tokens == 3 and C.sizeof(L.BeamPrefix) == 4


def test_hashable_by_the_width_alone():
    other = BeamPrefix(np.array([[1, 2, 3]], np.int32))
    assert PFX == other and hash(PFX) == hash(other) and PFX.key() == (3,) and PFX.ctx_key() == ('prefix', 3)
    assert PFX != BeamPrefix(np.array([[1, 2]], np.int32))


# ---- decoder.BeamOptions -----------------------------------------------------------------------------------------------------
def test_options_with_a_prefix_are_active_and_keep_the_six_tuple():
    assert BeamOptions(prefix=PFX).active and not BeamOptions().active
    assert BeamOptions().prefix is None
    for kw in (dict(), dict(length_penalty_weight=0.7), dict(constraints=BeamConstraints(min_length=2)),
               dict(sampling=BeamSampling(0.7, 3), truncation=BeamTruncation(5, 0.9))):
        with_p, without = BeamOptions(prefix=PFX, **kw), BeamOptions(**kw)
        assert with_p.ctx_key() == without.ctx_key() and len(with_p.ctx_key()) == 6
        assert without.context_key() == without.ctx_key()                       # prefix=None: the contexts of before
        assert with_p.context_key() == without.ctx_key() + (('prefix', 3),)
    # the context key differs by P and not by content
    same = BeamOptions(prefix=BeamPrefix(np.array([[1, 1, 1], [2, 2, 2]], np.int32)))
    wider = BeamOptions(prefix=BeamPrefix(np.array([[7, 9, -1, -1], [11, -1, -1, -1]], np.int32)))
    assert same.context_key() == BeamOptions(prefix=PFX).context_key() != wider.context_key()
    # appended after the existing fields: positional construction is what it was
    assert BeamOptions(0.7, None, None, None, None, None, None) == BeamOptions(length_penalty_weight=0.7)


def test_options_check_runs_the_prefix_check_in_its_place():
    rqd = BeamRequired(np.array([[[7]], [[9]]], np.int32))
    for kw in (dict(), dict(constraints=BeamConstraints(min_length=2, no_repeat_ngram=2)), dict(groups=BeamGroups(2, 0.5)),
               dict(sampling=BeamSampling(0.7, 3)), dict(sampling=BeamSampling(0.7, 3), truncation=BeamTruncation(5, 0.9)),
               dict(required=rqd), dict(required=rqd, length_penalty_weight=0.7), dict(length_penalty_weight=0.7)):
        BeamOptions(prefix=PFX, **kw).check(SPEC, 4, 2, 10)
    with pytest.raises(ValueError, match=r'max_tokens 3 is outside \[1,3\)'):
        BeamOptions(prefix=PFX).check(SPEC, 4, 2, 3)
    with pytest.raises(ValueError, match='the table holds 2 images, the batch 5'):
        BeamOptions(prefix=PFX).check(SPEC, 4, 5, 10)
    # consensus and the reward first, then the prefix, then truncation, required, groups, sampling, constraints
    broken = dict(prefix=BeamPrefix(np.array([[257]], np.int32)), truncation=BeamTruncation(-1), groups=BeamGroups(3, 0.5))
    with pytest.raises(ValueError, match='the table holds 1 images'):
        BeamOptions(**broken).check(SPEC, 4, 2, 10)
    with pytest.raises(ValueError, match='top_k'):
        BeamOptions(**dict(broken, prefix=PFX)).check(SPEC, 4, 2, 10)


def test_of_takes_the_prefix_keyword():
    defaults = dict(length_penalty_weight=0.0, groups=None, constraints=None, sampling=None, truncation=None, required=None,
                    consensus=None, image_base=0, prefix=None)
    assert BeamOptions.of(None, **dict(defaults, prefix=PFX)) == BeamOptions(prefix=PFX)
    with pytest.raises(ValueError, match='not both'):
        BeamOptions.of(BeamOptions(), **dict(defaults, prefix=PFX))


def test_prefix_log_probs_walks_the_parents():
    """Two images, W = 2, three steps.  Image 0 has a prefix of 2 tokens: slot 0 of the last step descends from slot 1 of
    step 1, so its prefix log-probability is that slot's score; image 1 has none: 0."""
    scores = np.array([[[-1.0, -9.0], [-0.5, -0.6]], [[-7.0, -2.0], [-1.5, -1.6]], [[-3.0, -8.0], [-2.5, -2.6]]], np.float32)
    parents = np.array([[[0, 0], [0, 0]], [[0, 0], [0, 1]], [[1, 0], [0, 1]]], np.int32)
    out = dict(scores=scores, parent_ids=parents, step_ids=np.zeros((3, 2, 2), np.int32))
    p = BeamPrefix(np.array([[4, 5], [-1, -1]], np.int32))
    np.testing.assert_array_equal(p.prefix_log_probs(out), np.array([[-2.0, -7.0], [0.0, 0.0]], np.float32))
    lp = p.prefix_log_probs(out, length_penalty_weight=1.0)
    np.testing.assert_allclose(lp[0], np.array([-2.0, -7.0]) * (7.0 / 6.0), rtol=1e-6)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_names_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
        m = re.search(r'\b%s\(' % name, header)
        assert m, name
        assert 'ops_rnn.py:49-112' in header[max(0, m.start() - 2500):m.start()], name
    assert '#define COMIC_ABI_VERSION 1' in header
    fields = re.search(r'typedef struct comic_beam_prefix \{(.*?)\} comic_beam_prefix;', re.sub(r'/\*.*?\*/', '', header, flags=re.S),
                       re.S).group(1)
    assert fields.split() == ['int32_t', 'max_tokens;']
    assert C.sizeof(L.BeamOptions) == 48                          # the prefix travels beside the record, not in it
    assert 'beam_prefix.hip' in open(os.path.join(ROOT, 'comic-compact-image-captioning-with-attention_amd', 'csrc', 'Makefile')).read()


def _descs(n, V):
    return (L.DecoderDesc * n)(*[cdec.DecoderSpec(V=V, **GOLDEN['spec']).desc(False) for _ in range(n)])


def _record(present, keep):
    structs = dict(constraints=L.BeamConstraints, groups=L.BeamGroups, sampling=L.BeamSampling, truncation=L.BeamTruncation,
                   required=L.BeamRequired)
    rec = L.BeamOptions()
    for name in present:
        keep.append(structs[name]())
        setattr(rec, name, C.addressof(keep[-1]))
    return rec


@pytest.mark.parametrize('n,rows,steps,V', list(itertools.product((1, 2), (8, 150), (6, 30), (258, 25599))))
def test_prefixed_workspace_query(n, rows, steps, V):
    """NULL prefix: the unprefixed query, byte for byte.  With a prefix: never less; exactly the mask block more where the
    decode has none of its own, and the same where constraints or a truncation allocate it already."""
    lib = L.load()
    descs = _descs(n, V)
    pfx = L.BeamPrefix(3)
    block = (rows * ((V + 31) // 32) * 4 + 255) // 256 * 256
    for present in ((), ('constraints',), ('groups',), ('sampling',), ('sampling', 'truncation'), ('required',),
                    ('constraints', 'required')):
        keep = []
        rec = _record(present, keep)
        plain = lib.comic_decoder_beam_search_workspace(descs, n, rows, steps, C.byref(rec))
        assert plain > 0
        assert lib.comic_decoder_beam_search_prefixed_workspace(descs, n, rows, steps, C.byref(rec), None) == plain
        got = lib.comic_decoder_beam_search_prefixed_workspace(descs, n, rows, steps, C.byref(rec), C.byref(pfx))
        assert got >= plain
        assert got == plain + (0 if ('constraints' in present or 'truncation' in present) else block), present
    assert lib.comic_decoder_beam_search_prefixed_workspace(descs, n, rows, steps, None, None) == \
        lib.comic_decoder_beam_search_workspace(descs, n, rows, steps, None)
    for bad in (0, steps, steps + 4, -1):
        p = L.BeamPrefix(bad)
        assert lib.comic_decoder_beam_search_prefixed_workspace(descs, n, rows, steps, None, C.byref(p)) == -1


@pytest.mark.parametrize('max_tokens,table,what', [
    (3, None, 'null prefix table'), (0, 0x1000, r'max_tokens 0 outside [1,6)'), (6, 0x1000, r'max_tokens 6 outside [1,6)'),
    (-2, 0x1000, r'max_tokens -2 outside [1,6)'),
])
def test_the_entry_refuses_an_illegal_prefix_before_it_reads_anything_else(max_tokens, table, what):
    """With null descs (and every other pointer null): a legal prefix gets as far as the null-pointer check, an illegal one
    is refused with its own message first."""
    lib = L.load()

    def call(prefix, tab):
        return lib.comic_decoder_beam_search_prefixed(None, None, None, None, None, 1, 2, 4, 6, None, prefix, tab, None, None,
                                                      None, None, None, None, None, None, 0, None)
    p = L.BeamPrefix(max_tokens)
    assert call(C.byref(p), table) != 0
    assert what in lib.comic_last_error().decode(), lib.comic_last_error()
    legal = L.BeamPrefix(5)
    for prefix, tab in ((C.byref(legal), 0x1000), (None, None), (None, 0x1000)):
        assert call(prefix, tab) != 0 and 'beam_ensemble: null pointer' in lib.comic_last_error().decode()
    keep = []
    rec = _record(('truncation',), keep)                           # an illegal record is still refused with a prefix beside it
    assert lib.comic_decoder_beam_search_prefixed(None, None, None, None, None, 1, 2, 4, 6, C.byref(rec), C.byref(legal), 0x1000,
                                                  None, None, None, None, None, None, None, None, 0, None) != 0
    assert 'null sampling' in lib.comic_last_error().decode()


def test_the_raw_operator_refuses_bad_arguments_on_the_host():
    lib = L.load()
    for args, what in (((None, 0x1000, 0x1000, 0, 1, 1, 33, 2, 0), 'null pointer'),
                       ((0x1000, None, 0x1000, 0, 1, 1, 33, 2, 0), 'null pointer'),
                       ((0x1000, 0x1000, None, 0, 1, 1, 33, 2, 0), 'null pointer'),
                       ((0x1000, 0x1000, 0x1000, 0, 0, 1, 33, 2, 0), 'bad shape'),
                       ((0x1000, 0x1000, 0x1000, 0, 1, 65, 33, 2, 0), 'bad shape'),
                       ((0x1000, 0x1000, 0x1000, 0, 1, 1, 65537, 2, 0), 'mask words'),
                       ((0x1000, 0x1000, 0x1000, 0, 1, 1, 0, 2, 0), 'mask words'),
                       ((0x1000, 0x1000, 0x1000, 0, 1, 1, 33, 0, 0), 'table width 0'),
                       ((0x1000, 0x1000, 0x1000, -1, 1, 1, 33, 2, 0), 'step -1 is negative'),
                       ((0x1000, 0x1000, 0x1004, 0, 1, 1, 33, 2, 0), '16-byte aligned')):
        assert lib.comic_beam_prefix_mask(*args, None) != 0
        assert what in lib.comic_last_error().decode(), (what, lib.comic_last_error())


# ---- the rule in numpy ---------------------------------------------------------------------------------------------------------
def test_the_numpy_rule_on_hand_made_rows():
    """B = 2, W = 2, V = 35: image 0 is forced to token 33 at step 1, image 1 is past its prefix; slot 1 of image 0 is
    finished.  The forced row bans everything below V but 33 -- its constraint bans included --, the finished row nothing,
    and image 1 keeps the constraints' mask."""
    V, W = 35, 2
    pfx = np.array([[4, 33, -1], [6, -1, -1]], np.int32)
    cons = np.zeros((4, V), bool)
    cons[:, 33] = True                                            # the constraints ban the very token the prefix forces
    cons[:, 2] = True
    fin = np.array([0, 1, 0, 0], np.int32)
    m = pref.forced_mask(cons, pfx, fin, 1, W)
    assert m[0].sum() == V - 1 and not m[0, 33]
    assert not m[1].any()
    np.testing.assert_array_equal(m[2:], cons[2:])
    bits = pack_bits(m)
    assert bits.shape == (4, 2) and bits[0, 0] == 0xffffffff and bits[0, 1] == 0b101        # bits 32 and 34; none at >= V
    np.testing.assert_array_equal(pref.forced_mask(cons, pfx, fin, 3, W)[[0, 2, 3]], cons[[0, 2, 3]])      # t >= P: nobody
    out_of_range = np.array([[4, 99, -1], [6, -1, -1]], np.int32)                # an entry outside [0, V) forces nobody
    np.testing.assert_array_equal(pref.forced_mask(cons, out_of_range, fin, 1, W)[0], cons[0])
    assert pref.prefix_lengths(pfx).tolist() == [2, 1]


# ---- the configuration and the command line ---------------------------------------------------------------------------------
WTOI = {'a': 0, 'close': 1, 'up': 2, 'of': 3, '<GO>': 4, '<EOS>': 5, 'dog': 6, '<PAD>': 7}
FILES = ['COCO_val2014_000000000042.jpg', 'dir/COCO_val2014_000000000007.jpg', 'x/COCO_val2014_000000000009.jpg']


def _config(**kw):
    return SimpleNamespace(**dict(dict(infer_beam_size=4, infer_max_length=20, token_type='word', radix_base=256, wtoi=WTOI), **kw))


def test_no_flag_no_prefix_and_the_suffix_is_unchanged():
    c = _config(infer_min_length=3)
    assert cdec.prefix_from_config(c) is None and cdec.prefix_from_config(c, FILES) is None
    assert cdec.prefix_dir_suffix(c) == ''
    assert cdec.decode_dir_suffix(c) == (cdec.constraints_dir_suffix(c) + cdec.groups_dir_suffix(c) + cdec.sampling_dir_suffix(c)
                                         + cdec.truncation_dir_suffix(c) + cdec.consensus_dir_suffix(c)
                                         + cdec.required_dir_suffix(c)) == '_min3_ngram0_sup0'
    assert cdec.options_from_config(c).prefix is None


def test_one_prefix_for_every_image_on_word_tokens():
    c = _config(infer_prefix='a close up of', infer_min_length=3)
    assert cdec.prefix_from_config(c) == dict(stride=1)
    out = cdec.prefix_from_config(c, FILES, max_steps=20)
    np.testing.assert_array_equal(out['prefix'].ids, np.tile(np.array([0, 1, 2, 3], np.int32), (3, 1)))
    assert out['words'] == [['a', 'close', 'up', 'of']] * 3 and out['cut'] == [[]] * 3
    assert cdec.prefix_dir_suffix(c) == '_pfx_a-close-up-of'
    assert cdec.decode_dir_suffix(c) == '_min3_ngram0_sup0_pfx_a-close-up-of'          # appended last
    assert cdec.options_from_config(c).prefix is None                                   # the rows come per batch
    for word, what in (('cat', "'cat' is outside the vocabulary"), ('<EOS>', "'<EOS>' is a special token")):
        with pytest.raises(ValueError, match=what):
            cdec.options_from_config(_config(infer_prefix='a ' + word), load=False)
    with pytest.raises(ValueError, match='4 tokens do not leave a step of the 4'):
        cdec.prefix_from_config(c, FILES, max_steps=4)


def test_radix_tokens_are_a_stride_of_tokens_per_word():
    from comic_amd.ops import build_radix_wtoi
    wtoi = dict(WTOI, **{'<PAD>': -1})                              # (the radix vocabulary keeps <PAD> at -1)
    c = _config(infer_prefix='up dog', token_type='radix', radix_base=2, wtoi=wtoi)
    enc = build_radix_wtoi(wtoi, 2)
    S = len(enc['a'])
    assert S == 4 and cdec.prefix_from_config(c) == dict(stride=4)
    out = cdec.prefix_from_config(c, FILES[:1], max_steps=30)
    assert out['prefix'].ids.tolist() == [enc['up'] + enc['dog']] and out['prefix'].max_tokens == 2 * S
    with pytest.raises(ValueError, match='8 tokens do not leave a step of the 8'):
        cdec.prefix_from_config(c, FILES[:1], max_steps=8)


def test_a_file_of_prefixes_by_name_and_by_image_id(tmp_path):
    path = tmp_path / 'starts.json'
    path.write_text(json.dumps({'COCO_val2014_000000000042.jpg': 'a close up', '7': ['a', 'dog', 'cat', 'of'], 'nobody.jpg': 'a'}))
    c = _config(infer_prefix_file=str(path))
    assert cdec.prefix_from_config(c) == dict(stride=1)
    out = cdec.prefix_from_config(c, FILES, max_steps=20)
    assert out['words'] == [['a', 'close', 'up'], ['a', 'dog'], []]
    assert out['cut'] == [[], ['cat', 'of'], []]                                    # cut before the first unknown word
    np.testing.assert_array_equal(out['prefix'].ids, np.array([[0, 1, 2], [0, 6, -1], [-1, -1, -1]], np.int32))
    out['prefix'].check(SimpleNamespace(V=len(WTOI), end_id=5, start_id=4), 3, 3, 20)
    assert cdec.prefix_dir_suffix(c) == '_pfx_starts' and cdec.decode_dir_suffix(c) == '_pfx_starts'
    with pytest.raises(ValueError, match='the longest prefix, 3 tokens, does not leave a step of the 3'):
        cdec.prefix_from_config(c, FILES, max_steps=3)
    path.write_text(json.dumps({'1': 5}))
    with pytest.raises(ValueError, match='must hold a JSON object of image -> string or list of words'):
        cdec.prefix_from_config(c)


def test_both_flags_and_char_tokens_are_refused(tmp_path):
    path = tmp_path / 'starts.json'
    path.write_text('{}')
    both = _config(infer_prefix='a', infer_prefix_file=str(path))
    for f in (cdec.prefix_from_config, cdec.prefix_dir_suffix, cdec.decode_dir_suffix, lambda c: cdec.options_from_config(c, load=False)):
        with pytest.raises(ValueError, match='give one of them, not both'):
            f(both)
    for kw in (dict(infer_prefix='a'), dict(infer_prefix_file=str(path))):
        with pytest.raises(ValueError, match='needs `word` or `radix` tokens, not `char`'):
            cdec.options_from_config(_config(token_type='char', **kw), load=False)


def test_the_command_line_has_the_two_flags():
    sp = importlib.util.spec_from_file_location('cli_infer_prefix', os.path.join(ROOT, 'src', 'infer.py'))
    cli = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(cli)
    parser = cli.create_parser()
    base = ['--infer_checkpoints_dir', 'x']
    args = parser.parse_args(base)
    assert args.infer_prefix is None and args.infer_prefix_file is None
    args = parser.parse_args(base + ['--infer_prefix', 'a close up of', '--infer_prefix_file', 'p.json'])
    assert (args.infer_prefix, args.infer_prefix_file) == ('a close up of', 'p.json')
