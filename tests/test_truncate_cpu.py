"""Host side of the top-k / nucleus truncation of the sampled step, no GPU: the float64 reference of
tests/beam_truncate_ref.py on hand-made rows, BeamTruncation's checks, the struct, the new entries in the header and the
bindings, the infer.py flags and the directory name."""
import ctypes as C
import importlib.util
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import comic_amd._lib as L
from comic_amd import decoder as cdec
from comic_amd.decoder import BeamSampling, BeamTruncation
from tests import beam_truncate_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('comic_beam_truncate_workspace', 'comic_beam_truncate', 'comic_decoder_beam_truncated_workspace',
               'comic_decoder_beam_truncated')


# ---- the reference on hand-made rows -----------------------------------------------------------------------------------
def _row(p, top_k=0, top_p=1.0, banned=()):
    a = np.log(np.asarray(p, np.float64))
    allowed = np.ones(a.size, bool)
    allowed[list(banned)] = False
    return tref.truncate_row(a, allowed, top_k, top_p)


def _kept(r):
    return np.flatnonzero(r['exact']).tolist()


def test_top_k_1_keeps_the_argmax_and_a_full_k_keeps_everything():
    p = [0.1, 0.4, 0.2, 0.3]
    assert _kept(_row(p, top_k=1)) == [1]
    assert _kept(_row(p, top_k=2)) == [1, 3]
    assert _kept(_row(p, top_k=4)) == [0, 1, 2, 3] and _kept(_row(p, top_k=9)) == [0, 1, 2, 3]
    assert _kept(_row(p, top_k=0, top_p=1.0)) == [0, 1, 2, 3]
    r = _row(p, top_k=2)
    assert r['k_clear'] and (r['must_keep'] == r['exact']).all() and (r['must_drop'] == ~r['exact']).all()


def test_top_p_takes_the_smallest_prefix_that_reaches_p():
    p = [0.1, 0.4, 0.2, 0.3]
    assert _kept(_row(p, top_p=0.3)) == [1]
    assert _kept(_row(p, top_p=0.5)) == [1, 3]                  # 0.4 < 0.5 <= 0.7
    assert _kept(_row(p, top_p=0.8)) == [1, 2, 3]
    assert _kept(_row(p, top_p=0.95)) == [0, 1, 2, 3]
    # a mass within GAP of top_p is the band: 0.4 + 0.3 against 0.7
    r = _row(p, top_p=0.7)
    assert np.flatnonzero(r['must_keep']).tolist() == [1, 3] and np.flatnonzero(~r['must_keep'] & ~r['must_drop']).tolist() == [2]


def test_banned_tokens_count_neither_in_k_nor_in_z():
    p = [0.1, 0.4, 0.2, 0.3]
    assert _kept(_row(p, top_k=2, banned=[1])) == [2, 3]
    assert _kept(_row(p, top_k=3, banned=[1])) == [0, 2, 3] and _row(p, top_k=3, banned=[1])['n_allowed'] == 3
    # without token 1 the rest renormalises to 1/6, 2/6, 3/6: 0.5 is reached by token 3 alone, 0.6 needs token 2 as well
    assert _kept(_row(p, top_p=0.45, banned=[1])) == [3]
    assert _kept(_row(p, top_p=0.6, banned=[1])) == [2, 3]
    r = _row(p, top_p=0.6, banned=[1])
    assert r['must_drop'][1] and not r['must_keep'][1]
    assert _row(p, top_k=1, banned=[0, 1, 2, 3]) is None                     # all banned: left as it came


def test_tie_rules():
    p = [0.2, 0.2, 0.2, 0.1, 0.2, 0.1]
    assert _kept(_row(p, top_k=2)) == [0, 1]                   # top-k: the lowest v among the tied
    assert not _row(p, top_k=2)['k_clear']
    assert _kept(_row(p, top_k=5)) == [0, 1, 2, 3, 4]
    assert _kept(_row(p, top_p=0.3)) == [0, 1, 2, 4]           # top-p: the whole tie group at the boundary
    assert _kept(_row(p, top_p=0.85)) == [0, 1, 2, 3, 4, 5]
    assert _kept(_row(p, top_k=3, top_p=0.5)) == [0, 1, 2]     # k first (lowest v), then the group of what is left
    # the nucleus is taken on the distribution renormalised over K
    q = [0.5, 0.3, 0.1, 0.1]
    assert _kept(_row(q, top_p=0.85)) == [0, 1, 2, 3] and _kept(_row(q, top_k=2, top_p=0.85)) == [0, 1]
    assert _kept(_row(q, top_k=2, top_p=0.6)) == [0]


def test_rows_left_as_they_came_and_the_whole_reference():
    lp = np.log(np.array([[[0.1, 0.4, 0.2, 0.3], [0.25, 0.25, 0.25, 0.25]]]))
    ref = tref.truncate_ref(lp, np.array([[0, 1]]), 1.0, 1, 1.0)
    assert ref['rows'][0, 1] is None and _kept(ref['rows'][0, 0]) == [1]
    assert ref['band'] == 0 and ref['k_clear'] and ref['keep_min'] == 1
    dropped = np.array([[[True, False, True, True], [False] * 4]])
    tref.check_mask(dropped, ref, 1, 1.0, exact=True)
    with pytest.raises(AssertionError):
        tref.check_mask(~dropped, ref, 1, 1.0)
    nan = lp.copy()
    nan[0, 0, 2] = np.nan
    assert tref.truncate_ref(nan, np.array([[0, 0]]), 1.0, 1, 1.0)['rows'][0, 0] is None
    bits = np.array([[0b1101, 0]], np.uint32)
    assert tref.unpack_bits(bits, 4).tolist() == [[True, False, True, True]]
    with pytest.raises(AssertionError):
        tref.unpack_bits(bits, 2)


# ---- BeamTruncation ----------------------------------------------------------------------------------------------------
def test_defaults_and_identity():
    t = BeamTruncation()
    assert not t.active and t.key() == (0, 1.0)
    assert BeamTruncation(40).active and BeamTruncation(top_p=0.9).active and not BeamTruncation(0, 1.5).active
    assert BeamTruncation(40, 0.9) == BeamTruncation('40', '0.9') and BeamTruncation(40, 0.9) != BeamTruncation(40, 0.8)
    assert len({BeamTruncation(40, 0.9), BeamTruncation(40, 0.9), BeamTruncation(5, 0.9)}) == 2
    assert repr(BeamTruncation(40, 0.9)) == 'BeamTruncation(top_k=40, top_p=0.9)'
    assert BeamTruncation(40, 0.9).ctx_key() != BeamTruncation(41, 0.9).ctx_key() != BeamTruncation(41, 0.8).ctx_key()
    assert BeamTruncation(40, 0.9).ctx_key() == ('truncate', 40, float(np.float32(0.9)))
    BeamTruncation(40, 0.9).check(BeamSampling(0.7, 3))
    BeamTruncation().check(None)                                # inactive: nothing to refuse


@pytest.mark.parametrize('kw,sampling,field', [
    (dict(top_k=-1), BeamSampling(), 'top_k'),
    (dict(top_p=0.0), BeamSampling(), 'top_p'),
    (dict(top_p=-0.5), BeamSampling(), 'top_p'),
    (dict(top_p=float('nan')), BeamSampling(), 'top_p'),
    (dict(top_k=5), None, 'sampling'),
    (dict(top_p=0.9), BeamSampling(enabled=False), 'sampling'),
])
def test_check_refuses(kw, sampling, field):
    with pytest.raises(ValueError, match=field):
        BeamTruncation(**kw).check(sampling)


def test_beam_sampling_is_unchanged():
    assert BeamSampling(0.7, 3).ctx_key() == ('sample', float(np.float32(0.7)))
    assert BeamSampling(0.7, 3).key() == (0.7, 3, True)
    assert repr(BeamSampling(0.7, 3)) == 'BeamSampling(temperature=0.7, seed=3)'


def test_struct_matches_the_header():
    assert C.sizeof(L.BeamTruncation) == 8
    s = BeamTruncation(40, 0.5).c_struct()
    assert (s.top_k, s.top_p) == (40, 0.5)
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    assert re.search(r'typedef struct comic_beam_truncation \{\s*int32_t top_k;\s*float top_p;\s*\} comic_beam_truncation;',
                     header)


def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS
        m = re.search(r'\b%s\(' % name, header)
        assert m, name
        assert 'ops_rnn.py:49-112' in header[max(0, m.start() - 1500):m.start()], name
    assert '#define COMIC_ABI_VERSION 1' in header               # additive change
    lib = L.load()
    assert lib.comic_beam_truncate_workspace(0, 2, 3, 17) == -1
    assert lib.comic_beam_truncate_workspace(1, 2, 3, 65537) == -1
    assert lib.comic_beam_truncate_workspace(1, 50, 5, 25599) == 0           # the row's keys stay in LDS
    assert lib.comic_beam_truncate_workspace(1, 1, 2, 65536) == 2 * 65536 * 4      # a scratch row per slot


# ---- configuration and CLI -----------------------------------------------------------------------------------------------
def _infer_cli():
    spec = importlib.util.spec_from_file_location('cli_infer_truncate_flags', os.path.join(ROOT, 'src', 'infer.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_infer_flags_are_absent_by_default_and_parsed_when_given():
    parser = _infer_cli().create_parser()
    overlay = {k: v for k, v in parser.parse_args([]).__dict__.items() if v is not None}
    assert not {'infer_top_k', 'infer_top_p'} & set(overlay)
    args = parser.parse_args(['--infer_sample', '--infer_temperature', '0.7', '--infer_top_k', '5', '--infer_top_p', '0.9'])
    assert (args.infer_sample, args.infer_top_k, args.infer_top_p) == (True, 5, 0.9)


def test_truncation_from_config():
    ns = SimpleNamespace
    assert cdec.truncation_from_config(ns(infer_beam_size=5)) is None
    assert cdec.truncation_from_config(ns(infer_beam_size=5, infer_sample=True, infer_top_k=None, infer_top_p=None)) is None
    assert cdec.truncation_from_config(ns(infer_beam_size=5, infer_sample=True, infer_top_k=40, infer_top_p=0.9)) \
        == BeamTruncation(40, 0.9)
    assert cdec.truncation_from_config(ns(infer_beam_size=5, infer_sample=True, infer_top_k=40)) == BeamTruncation(40, 1.0)
    assert cdec.truncation_from_config(ns(infer_beam_size=5, infer_sample=True, infer_top_p=0.9)) == BeamTruncation(0, 0.9)
    for kw in (dict(infer_top_k=40), dict(infer_top_p=0.9), dict(infer_top_k=40, infer_temperature=0.7)):
        with pytest.raises(ValueError, match='infer_sample'):
            cdec.truncation_from_config(ns(infer_beam_size=5, **kw))
    with pytest.raises(ValueError, match='top_k'):
        cdec.truncation_from_config(ns(infer_beam_size=5, infer_sample=True, infer_top_k=-2))
    with pytest.raises(ValueError, match='top_p'):
        cdec.truncation_from_config(ns(infer_beam_size=5, infer_sample=True, infer_top_p=0.0))


def test_directory_suffix():
    parser = _infer_cli().create_parser()
    sfx = cdec.truncation_dir_suffix
    assert sfx(parser.parse_args([])) == ''
    assert sfx(parser.parse_args(['--infer_sample'])) == ''
    smp = ['--infer_sample', '--infer_temperature', '0.7', '--infer_sample_seed', '3']
    assert sfx(parser.parse_args(smp + ['--infer_top_k', '40', '--infer_top_p', '0.9'])) == '_k40_p0.9'
    assert sfx(parser.parse_args(smp + ['--infer_top_k', '40'])) == '_k40'
    assert sfx(parser.parse_args(smp + ['--infer_top_p', '0.9'])) == '_p0.9'
    both = parser.parse_args(smp + ['--infer_top_k', '5', '--infer_top_p', '0.9'])
    assert cdec.sampling_dir_suffix(both) + sfx(both) == '_smp_t0.7_s3_k5_p0.9'
    every = parser.parse_args(smp + ['--infer_min_length', '8', '--infer_top_k', '5'])
    assert cdec.constraints_dir_suffix(every) + cdec.groups_dir_suffix(every) + cdec.sampling_dir_suffix(every) + sfx(every) \
        == '_min8_ngram0_sup0_smp_t0.7_s3_k5'
