"""Consensus (minimum-Bayes-risk) selection without a GPU: the float64 reference of tests/consensus_ref.py against the host
scorer's restatement (oracle.scorer_ref.CiderD) and against hand-worked cases, the idf table builder, the host-side refusals,
the configuration, the directory suffixes and the header."""
import importlib.util
import math
import os
import pickle
import re
from types import SimpleNamespace

import numpy as np
import pytest

import comic_amd._lib as L
from comic_amd import decoder as cdec
from comic_amd.decoder import Consensus, NgramIdf
from oracle.scorer_ref import CiderD
from tests import consensus_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = 0
NEW_SYMBOLS = ('comic_caption_consensus_workspace', 'comic_caption_consensus')


def _rows(*cands, T=None):
    """Candidates given as token lists -> ids [T, 1, W], END padded."""
    T = T or max(len(c) for c in cands) + 1
    ids = np.full((T, 1, len(cands)), END, np.int32)
    for w, c in enumerate(cands):
        ids[:len(c), 0, w] = c
    return ids


def _pair_sim(a, b, stride=1, **kw):
    return cr.sim(cr.vectors(a, END, stride, **kw), cr.vectors(b, END, stride, **kw))


# ---- the reference against the host scorer ---------------------------------------------------------------------------------
@pytest.mark.parametrize('seed,V,T,W', [(0, 8, 12, 6), (1, 5, 20, 9), (2, 30, 9, 3)])
def test_reference_equals_the_host_scorer_on_ids_rendered_as_words(seed, V, T, W):
    """Hypothesis = one candidate, references = its siblings; ids as the words `w<id>`, stride 1, a random df dict."""
    rng = np.random.default_rng(seed)
    B = 3
    ids = rng.integers(1, V, (T, B, W))
    for b in range(B):
        for w in range(W):
            ids[rng.integers(0, T + 1):, b, w] = END
    ids[:, 0, 0] = END                                          # an empty candidate
    ids[:, 1, W - 1] = ids[:, 1, 0]                             # a duplicate
    df = {}
    for _ in range(80):
        ng = tuple(int(x) for x in rng.integers(1, V, rng.integers(1, 5)))
        df[ng] = float(rng.integers(0, 9))
    ref_len = 11
    util, best = cr.consensus(ids, END, 1, None, cr.df_table(df, ref_len), math.log(ref_len))
    scorer = CiderD({tuple('w%d' % x for x in ng): v for ng, v in df.items()}, ref_len)
    plain = CiderD({}, ref_len)
    util1, _ = cr.consensus(ids, END, 1)
    for b in range(B):
        text = [' '.join('w%d' % u[0] for u in cr.units(ids[:, b, w], END, 1)) for w in range(W)]
        for w in range(W):
            sib = [text[j] for j in range(W) if j != w]
            assert abs(util[b, w] - scorer.score_one(text[w], sib)) <= 1e-12
            # without a table every n-gram weighs 1: the scorer with an empty df, over log(ref_len)^2 per order ...
            # (norms cancel the scale): the same number
            assert abs(util1[b, w] - plain.score_one(text[w], sib)) <= 1e-12
        assert best[b] == int(np.argmax(util[b]))


# ---- hand-worked cases --------------------------------------------------------------------------------------------------------
def test_identical_candidates_score_ten():
    a = [3, 4, 5, 6, 7, END]
    assert abs(_pair_sim(a, a) - 10.0) <= 1e-12
    util, best = cr.consensus(_rows(a[:-1], a[:-1]), END)
    assert np.allclose(util, 10.0, atol=1e-12) and best[0] == 0          # the lowest slot on a tie


def test_disjoint_and_empty_candidates_score_zero():
    assert _pair_sim([1, 2, 3, 4, END], [5, 6, 7, 8, END]) == 0.0
    assert _pair_sim([END, END, END], [5, 6, 7, END]) == 0.0
    assert _pair_sim([5, 6, 7, END], [END, END, END]) == 0.0
    assert _pair_sim([END], [END]) == 0.0
    util, best = cr.consensus(_rows([], [5, 6, 7]), END)
    assert (util == 0.0).all() and best[0] == 0


def test_one_unit_against_one_unit():
    """U = 1: one unigram, no higher order, len = 0 on both sides: val_1 = 1, the others 0, sim = 10 / 4."""
    assert abs(_pair_sim([7, END], [7, END]) - 2.5) <= 1e-15
    assert _pair_sim([7, END], [8, END]) == 0.0
    # against two units: the unigram cosine 1 / sqrt(2), the length penalty exp(-1 / 72)
    want = 10.0 / 4.0 * (1.0 / math.sqrt(2.0)) * math.exp(-1.0 / 72.0)
    assert abs(_pair_sim([7, END], [7, 9, END]) - want) <= 1e-15


def test_term_frequency_clips():
    """h = a a a, r = a b: unigram vec_h[a] = 3, vec_r[a] = 1: min(3, 1) * 1 / (3 * sqrt(2)); len 2 against 1."""
    want = 10.0 / 4.0 * (1.0 / (3.0 * math.sqrt(2.0))) * math.exp(-1.0 / 72.0)
    assert abs(_pair_sim([1, 1, 1, END], [1, 2, END]) - want) <= 1e-15


def test_a_trailing_partial_word_is_ignored_at_stride_three():
    full = [1, 2, 3, 4, 5, 6, END, END, END]
    part = [1, 2, 3, 4, 5, 6, 7, 8, END]
    assert cr.units(part, END, 3) == [(1, 2, 3), (4, 5, 6)] == cr.units(full, END, 3)
    assert abs(_pair_sim(full, part, stride=3) - _pair_sim(full, full, stride=3)) == 0.0
    assert cr.units([1, 2, END], END, 3) == []
    # a unit is its tokens in order: (1, 2, 3) is not (3, 2, 1), and a word is not its halves
    assert _pair_sim([1, 2, 3, END], [3, 2, 1, END], stride=3) == 0.0
    assert cr.ngram_key([1, 2]) != cr.ngram_key([2, 1]) and cr.ngram_key([1]) != cr.ngram_key([1, 0])


def test_posterior_weights_and_dead_slots():
    ids = _rows([1, 2, 3], [1, 2, 4], [1, 2, 3], [9, 9, 9])
    lp = np.array([[-1.0, -2.0, -np.inf, -0.5]], np.float32)
    util, best = cr.consensus(ids, END, 1, lp)
    assert np.isneginf(util[0, 2]) and np.isfinite(util[0, [0, 1, 3]]).all()
    pi = np.exp(np.array([-1.0, -2.0, -0.5]) + 0.5)
    s01 = _pair_sim(ids[:, 0, 0], ids[:, 0, 1])
    assert abs(util[0, 0] - pi[1] * s01 / (pi[1] + pi[2])) <= 1e-14            # slot 2 does not vote, slot 3 shares nothing
    assert best[0] == int(np.argmax(np.where(np.isfinite(util[0]), util[0], -1)))
    util, best = cr.consensus(ids, END, 1, np.full((1, 4), -np.inf, np.float32))
    assert np.isneginf(util).all() and best[0] == 0
    util, best = cr.consensus(_rows([1, 2, 3]), END)                              # W = 1: a zero denominator
    assert util[0, 0] == 0.0 and best[0] == 0


# ---- the hash and the table -----------------------------------------------------------------------------------------------------
def test_the_hash_is_splitmix64_of_the_header():
    src = open(os.path.join(ROOT, 'comic-compact-image-captioning-with-attention_amd', 'csrc', 'splitmix.h')).read()
    for const in ('0x9E3779B97F4A7C15', '0xBF58476D1CE4E5B9', '0x94D049BB133111EB'):
        assert const in src
    assert int(cr.splitmix64(0)) == 0xE220A8397B1DCDAF                   # the generator's published first output for seed 0
    toks = np.array([[5, 6, 7], [1, 0, 300]])
    assert cdec.ngram_keys(toks).tolist() == [cr.ngram_key(t) for t in toks.tolist()]


def test_table_from_document_frequency():
    enc = {'a': [1], 'b': [2], 'c': [3], '<EOS>': [0], '<GO>': [9], '<PAD>': [8]}
    df = {('a',): 4.0, ('b',): 1.0, ('a', 'b'): 2.0, ('a', 'b', 'c'): 0.0, ('c', 'a', 'b', 'a'): 3.0,
          ('a', '<EOS>'): 5.0, ('<GO>', 'a'): 5.0, ('<PAD>',): 1.0, ('zebra', 'a'): 2.0}
    idf = NgramIdf.from_document_frequency(df, 10, enc, 1)
    assert (idf.kept, idf.skipped, idf.stride) == (5, 4, 1)
    assert idf.cap == 16 and idf.cap >= 2 * idf.kept and idf.cap & (idf.cap - 1) == 0
    assert int((idf.keys != 0).sum()) == 5 and idf.log_ref_len == math.log(10.0)
    for ng, cnt in list(df.items())[:5]:
        g = cr.table_lookup((idf.keys, idf.g), cr.ngram_key([enc[w][0] for w in ng]), None)
        assert g == math.log(10.0) - math.log(max(1.0, cnt)), ng
    assert cr.table_lookup((idf.keys, idf.g), cr.ngram_key([2, 1]), 'missing') == 'missing'
    # the device's table is the reference builder's table: the same weights for every candidate
    ids = _rows([1, 2, 3, 1, 2], [3, 1, 2, 1], [2, 2])
    mine = cr.consensus(ids, END, 1, None, (idf.keys, idf.g), idf.log_ref_len)[0]
    theirs = cr.consensus(ids, END, 1, None, cr.df_table({tuple(enc[w][0] for w in ng): c for ng, c in list(df.items())[:5]}, 10),
                          math.log(10.0))[0]
    np.testing.assert_array_equal(mine, theirs)


def test_table_at_stride_two_and_a_larger_dictionary():
    rng = np.random.default_rng(3)
    words = ['w%d' % i for i in range(40)]
    enc = {w: [i // 7, i % 7] for i, w in enumerate(words)}
    df = {}
    for _ in range(300):
        df[tuple(words[i] for i in rng.integers(0, 40, rng.integers(1, 5)))] = float(rng.integers(1, 50))
    idf = NgramIdf.from_document_frequency(df, 50, enc, 2)
    assert idf.kept == len(df) and idf.skipped == 0 and idf.cap >= 2 * len(df) and idf.cap & (idf.cap - 1) == 0
    assert idf.cap < 4 * len(df)
    for ng, cnt in df.items():
        key = cr.ngram_key([t for w in ng for t in enc[w]])
        assert cr.table_lookup((idf.keys, idf.g), key, None) == math.log(50.0) - math.log(cnt)
    with pytest.raises(ValueError, match='stride'):
        NgramIdf.from_document_frequency({('w1',): 1.0}, 50, enc, 1)


def test_table_from_pickle_through_the_vocabulary(tmp_path):
    path = tmp_path / 'scst-words.p'
    with open(path, 'wb') as f:
        pickle.dump({'document_frequency': {('a',): 2.0, ('a', 'dog'): 1.0, ('dog', '<EOS>'): 2.0, ('cat',): 1.0}, 'ref_len': 3}, f, 2)
    c = SimpleNamespace(token_type='word', wtoi={'a': 4, 'dog': 5, '<EOS>': 1})
    idf = NgramIdf.from_pickle(str(path), c)
    assert (idf.kept, idf.skipped, idf.stride) == (2, 2, 1)
    assert cr.table_lookup((idf.keys, idf.g), cr.ngram_key([4, 5]), None) == math.log(3.0)
    with pytest.raises(ValueError, match='char'):
        NgramIdf.from_pickle(str(path), SimpleNamespace(token_type='char', wtoi={}))


# ---- Consensus -------------------------------------------------------------------------------------------------------------------
def test_defaults_and_identity():
    c = Consensus()
    assert (c.weights, c.stride, c.idf, c.sigma) == ('uniform', 1, None, 6.0)
    assert Consensus('posterior', 2) == Consensus('posterior', '2') and Consensus() != Consensus('posterior')
    assert len({Consensus(), Consensus(), Consensus(stride=2), Consensus(sigma=5.0)}) == 3
    idf = NgramIdf(np.zeros(2, np.uint64), np.zeros(2), 1.0, 1)
    assert Consensus(idf=idf) == Consensus(idf=idf) != Consensus()
    assert Consensus(idf=idf) != Consensus(idf=NgramIdf(np.zeros(2, np.uint64), np.zeros(2), 1.0, 1))
    assert repr(Consensus()) == "Consensus(weights='uniform', stride=1, idf=None, sigma=6.0)"
    Consensus().check(32, 64)
    Consensus(stride=3).check(1, 192)


@pytest.mark.parametrize('kw,beam,steps,field', [
    (dict(), 33, 20, 'beam'),
    (dict(), 0, 20, 'beam'),
    (dict(), 5, 65, 'max_steps'),                 # T = 64 * stride + 1 at stride 1: just past the header's 64 units
    (dict(stride=2), 5, 129, 'max_steps'),
    (dict(weights='map'), 5, 20, 'weights'),
    (dict(stride=0), 5, 20, 'stride'),
    (dict(stride=9), 5, 20, 'stride'),
    (dict(sigma=0.0), 5, 20, 'sigma'),
    (dict(sigma=float('nan')), 5, 20, 'sigma'),
    (dict(stride=2, idf=NgramIdf(np.zeros(2, np.uint64), np.zeros(2), 1.0, 1)), 5, 20, 'idf'),
])
def test_check_refuses(kw, beam, steps, field):
    with pytest.raises(ValueError, match=field):
        Consensus(**kw).check(beam, steps)


def test_the_c_entry_refuses_with_an_error_code_before_any_launch():
    """(No GPU is needed: every one of these returns before the launch.)"""
    lib = L.load()
    assert lib.comic_caption_consensus_workspace(50, 32, 64, 1) == 0
    assert lib.comic_caption_consensus_workspace(50, 32, 512, 8) == 0
    for B, W, T, stride in ((50, 33, 20, 1), (50, 0, 20, 1), (50, 5, 65, 1), (50, 5, 193, 3), (50, 5, 20, 0), (50, 5, 20, 9),
                            (0, 5, 20, 1), (50, 5, 0, 1)):
        assert lib.comic_caption_consensus_workspace(B, W, T, stride) == -1
        assert lib.comic_caption_consensus(None, T, B, W, 0, stride, None, 0, None, None, 0, 0.0, 6.0, None, None, None, 0,
                                           None) == 2
    assert lib.comic_caption_consensus(None, 65, 2, 5, 0, 1, None, 0, None, None, 0, 0.0, 6.0, None, None, None, 0, None) == 2
    assert 'T = 65' in lib.comic_last_error().decode()
    assert lib.comic_caption_consensus(None, 20, 2, 33, 0, 1, None, 0, None, None, 0, 0.0, 6.0, None, None, None, 0, None) == 2
    assert 'W = 33' in lib.comic_last_error().decode()


# ---- configuration and CLI -----------------------------------------------------------------------------------------------
def _infer_cli():
    spec = importlib.util.spec_from_file_location('cli_infer_consensus_flags', os.path.join(ROOT, 'src', 'infer.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _config(**kw):
    base = dict(infer_beam_size=5, infer_max_length=20, token_type='word', wtoi={'a': 4, 'dog': 5}, radix_base=256)
    base.update(kw)
    return SimpleNamespace(**base)


def test_infer_flags_are_absent_by_default_and_parsed_when_given():
    parser = _infer_cli().create_parser()
    overlay = {k: v for k, v in parser.parse_args([]).__dict__.items() if v is not None}
    assert not {'infer_consensus', 'infer_consensus_df'} & set(overlay)
    args = parser.parse_args(['--infer_sample', '--infer_consensus', '--infer_consensus_df', 'x.p'])
    assert (args.infer_sample, args.infer_consensus, args.infer_consensus_df) == (True, True, 'x.p')


def test_consensus_from_config(tmp_path):
    assert cdec.consensus_from_config(_config()) is None
    assert cdec.consensus_from_config(_config(infer_sample=True)) is None
    assert cdec.consensus_from_config(_config(infer_sample=True, infer_consensus=True)) == Consensus('uniform', 1)
    radix = _config(infer_sample=True, infer_consensus=True, token_type='radix', wtoi={'w%d' % i: i for i in range(300)})
    assert cdec.consensus_from_config(radix) == Consensus('uniform', 2)
    with pytest.raises(ValueError, match='infer_sample'):                       # the flag without --infer_sample
        cdec.consensus_from_config(_config(infer_consensus=True))
    with pytest.raises(ValueError, match='char'):
        cdec.consensus_from_config(_config(infer_sample=True, infer_consensus=True, token_type='char'))
    with pytest.raises(ValueError, match='infer_consensus'):
        cdec.consensus_from_config(_config(infer_sample=True, infer_consensus_df='x.p'))
    with pytest.raises(ValueError, match='beam'):
        cdec.consensus_from_config(_config(infer_sample=True, infer_consensus=True, infer_beam_size=33))
    with pytest.raises(ValueError, match='max_steps'):
        cdec.consensus_from_config(_config(infer_sample=True, infer_consensus=True, infer_max_length=65))
    with pytest.raises(ValueError, match='no file'):
        cdec.consensus_from_config(_config(infer_sample=True, infer_consensus=True, infer_consensus_df=str(tmp_path / 'none.p')))
    path = tmp_path / 'scst-words.p'
    with open(path, 'wb') as f:
        pickle.dump({'document_frequency': {('a',): 2.0, ('a', 'dog'): 1.0}, 'ref_len': 3}, f, 2)
    cfg = _config(infer_sample=True, infer_consensus=True, infer_consensus_df=str(path))
    cons = cdec.consensus_from_config(cfg)
    assert cons.idf.kept == 2 and cons.stride == 1
    assert cdec.consensus_from_config(cfg, load_idf=False).idf is None


def test_directory_suffix():
    parser = _infer_cli().create_parser()
    sfx = cdec.consensus_dir_suffix
    assert sfx(parser.parse_args([])) == ''
    assert sfx(parser.parse_args(['--infer_sample'])) == ''
    smp = ['--infer_sample', '--infer_temperature', '0.7', '--infer_sample_seed', '3']
    assert sfx(parser.parse_args(smp + ['--infer_consensus'])) == '_cns'
    both = parser.parse_args(smp + ['--infer_consensus', '--infer_consensus_df', '/data/x_scst-words.p', '--infer_top_k', '5'])
    assert sfx(both) == '_cns_df'
    assert cdec.sampling_dir_suffix(both) + cdec.truncation_dir_suffix(both) + sfx(both) == '_smp_t0.7_s3_k5_cns_df'


def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS
        assert re.search(r'\b%s\(' % name, header), name
    assert '#define COMIC_ABI_VERSION 1' in header               # additive change
    m = re.search(r'\bcomic_caption_consensus_workspace\(', header)
    doc = header[max(0, m.start() - 5000):m.start()]
    for word in ('U <= 64', 'W <= 32', '64-BIT KEYS', 'splitmix64', 'COMIC_CONSENSUS_POSTERIOR'):
        assert word in doc, word
    assert cdec.Consensus.MAX_W == 32 and cdec.Consensus.MAX_UNITS == 64
