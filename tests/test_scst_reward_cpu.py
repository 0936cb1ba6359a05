"""The SCST reward without a GPU: the float64 reference on word ids (tests/scst_reward_ref.py) against the host scorer's
restatement ON TEXT (oracle.scorer_ref.CaptionScorer) and against the native host scorer, the canonical words against
ops.id_to_caption, the packer and the extended vocabulary, Reward's refusals, the C entries' refusals, the flags and the
directory names.  The case builders serve tests/test_gpu_scst_reward.py too."""
import functools
import importlib.util
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import comic_amd._lib as L
from comic_amd import decoder as cdec, ops
from comic_amd.decoder import NgramIdf, Reward, RewardRefs, RewardVocab
from oracle import scorer_ref as sr
from tests import scst_reward_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('comic_scst_reward_workspace', 'comic_scst_reward', 'comic_scst_coefficients')
WORDS = ['a', 'b', 'c', 'd', 'e', 'f', 'g', 'h']
REF_LEN = 40
WEIGHTS = {'default': (1.0, (0.0, 0.0, 0.0, 2.0)), 'cider': (1.0, (0.0,) * 4), 'bleu': (0.0, (0.5, 0.25, 0.125, 1.0))}
# (token type, radix base): a 12-entry vocabulary gives word length 2 at base 4 and 3 at base 3
TOKENS = {'word': ('word', 0), 'radix4': ('radix', 4), 'radix3': ('radix', 3)}


def make_config(kind):
    """A 12-entry vocabulary: 8 words, <UNK>, <GO>, <EOS> with the ids 0..10 and <PAD> = -1; the id 11 = len - 1 is the one
    the table lacks."""
    token_type, base = TOKENS[kind]
    wtoi = {'<PAD>': -1}
    wtoi.update({w: i for i, w in enumerate(WORDS + ['<UNK>', '<GO>', '<EOS>'])})
    return SimpleNamespace(token_type=token_type, radix_base=base, wtoi=wtoi, itow={str(i): w for w, i in wtoi.items()})


def _spell(cfg, words, T):
    """The tokens of a caption of vocabulary words, then <EOS> to the end of the row."""
    if cfg.token_type == 'word':
        toks, eos = [cfg.wtoi[w] for w in words], cfg.wtoi['<EOS>']
    else:
        table = ops.build_radix_wtoi(cfg.wtoi, cfg.radix_base)
        toks, eos = [d for w in words for d in table[w]], cfg.radix_base + 1
    assert len(toks) <= T, (len(toks), T)
    return toks + [eos] * (T - len(toks))


@functools.lru_cache(maxsize=None)
def make_case(kind, T, W, R, B, seed=0, alphabet=8, T0=None):
    """-> namespace(cfg, ids [T,B,W], base_ids [T,B], refs [B][R_b] text, df (text), ...).  Image 0 has R references, two of
    them with the word `zebra` outside the vocabulary (its n-grams are in the df table); image 1 has one reference only.
    Rollout 0 of image 0 is empty, rollout 1 equals reference 0, the last repeats a bigram (tf > 1, BLEU clipping); the
    random rollouts hold tokens after their first <EOS>, negative tokens, odd digit counts and word ids >= the vocabulary.
    alphabet: the words the references and the `word` rollouts draw from (a small one makes n-grams repeat).  T0: the
    length of the baseline rows (default T)."""
    cfg = make_config(kind)
    words = WORDS[:alphabet]
    rng = np.random.default_rng(100 * T + 10 * W + R + seed)
    wl = 1 if cfg.token_type == 'word' else len(ops.number_to_base(len(cfg.itow), cfg.radix_base))
    max_words = max(1, min(10, T // wl))
    refs = []
    for b in range(B):
        n = R if b == 0 else (1 if b == 1 else int(rng.integers(1, R + 1)))
        refs.append([' '.join(rng.choice(words, int(rng.integers(1, max_words + 1)))) for _ in range(n)])
    if R >= 2:
        refs[0][0] = 'zebra ' + refs[0][0]
        refs[0][1] = refs[0][1] + ' zebra ' + refs[0][0].split()[1]
    df = sr.build_df_from_refs(refs + [[' '.join(rng.choice(words, 6)) for _ in range(3)] for _ in range(6)])
    df['ref_len'] = REF_LEN
    if cfg.token_type == 'word':
        eos = cfg.wtoi['<EOS>']
        ids = rng.integers(0, alphabet + 1 if alphabet == 8 else alphabet, (T, B, W))      # (the full alphabet: <UNK> too)
        ids[rng.random((T, B, W)) < 0.08] = -1
        ids[rng.random((T, B, W)) < 0.08] = cfg.wtoi['<GO>']
    else:
        eos = cfg.radix_base + 1
        ids = rng.integers(0, cfg.radix_base, (T, B, W))
        ids[rng.random((T, B, W)) < 0.06] = -1
        ids[rng.random((T, B, W)) < 0.06] = cfg.radix_base          # <GO>
    base_ids = ids[:, :, 0].copy()[rng.permutation(T)]
    if T0 is not None:                                                    # rows of another length: the tokens of the rollouts, cycled
        base_ids = np.stack([ids[t % T, :, (t // T) % W] for t in range(T0)])
    for b in range(B):
        for w in range(W):
            e = int(rng.integers(0, T + 1))
            ids[e:, b, w] = np.where(rng.random(T - e) < 0.8, eos, ids[e:, b, w])      # tokens after the first <EOS>
            if e < T:
                ids[e, b, w] = eos
    ids[:, 0, 0] = eos                                                   # an empty rollout
    own = [w for w in refs[0][0].split() if w != 'zebra'][:max_words]
    if W >= 2:
        ids[:, 0, 1] = _spell(cfg, own, T)                               # a reference, less the word outside the vocabulary
    if W >= 3 and T // wl >= 4:
        ids[:, 0, W - 1] = _spell(cfg, (['a', 'b'] * 8)[:min(6, T // wl)], T)
    if B >= 2 and W >= 2:
        ids[:, 1, 0] = _spell(cfg, refs[1][0].split()[:max_words], T)    # equal to the only reference
    return SimpleNamespace(cfg=cfg, ids=ids.astype(np.int32), base_ids=base_ids.astype(np.int32), refs=refs, df=df, T=T, W=W,
                           R=R, B=B, kind=kind)


def on_ids(case):
    """The case through the vocabulary: vocab, refs and df on word ids, the packed references."""
    vocab = RewardVocab(case.cfg)
    ref_ids = [[vocab.encode(r) for r in rl] for rl in case.refs]
    df_ids = {tuple(vocab.id(w) for w in ng): cnt for ng, cnt in case.df['document_frequency'].items()}
    return vocab, ref_ids, df_ids


def text_rows(case, rows):
    return ops.id_to_caption(np.asarray(rows), case.cfg, skip_unmapped=True)


CASES = [('word', 12, 7, 5, 5), ('word', 12, 2, 1, 2), ('radix4', 16, 5, 5, 3), ('radix3', 17, 4, 3, 3)]


# ---- the reference against the host scorer, on text ---------------------------------------------------------------------------
@pytest.mark.parametrize('weights', list(WEIGHTS))
@pytest.mark.parametrize('shape', CASES)
def test_reference_equals_the_host_scorer_on_text(shape, weights):
    case = make_case(*shape)
    w_c, w_b = WEIGHTS[weights]
    vocab, ref_ids, df_ids = on_ids(case)
    got = rr.score_ids(case.ids, ref_ids, vocab, df_ids, REF_LEN, w_c, w_b, rr.ROW, case.base_ids)
    T, B, W = case.ids.shape
    sample = [[s] for s in text_rows(case, case.ids.transpose(2, 1, 0).reshape(W * B, T))]      # hypothesis-major
    greedy = [[s] for s in text_rows(case, case.base_ids.T)]
    scorer = sr.CaptionScorer(case.df, dict(ciderD=w_c, bleu=list(w_b)))
    _, sc_sample, sc_greedy = scorer.get_hypo_scores(case.refs, sample, greedy)
    assert np.abs(got['reward'][:, :W].T.reshape(-1) - sc_sample).max() <= 1e-12
    assert np.abs(np.tile(got['reward'][:, W], W) - sc_greedy).max() <= 1e-12
    assert np.abs(got['advantage'].reshape(-1) - (sc_sample - sc_greedy).astype(np.float32)).max() <= 1e-6
    for b in range(B):
        for w in range(W):
            if w_c > 0:
                assert abs(got['cider'][b, w] - scorer.cider.score_one(sample[w * B + b][0], case.refs[b])) <= 1e-12
            else:
                assert got['cider'][b, w] == 0.0
            if max(w_b) > 0:
                assert np.abs(got['bleu'][b, w] - sr.bleu_sentence_scores(sample[w * B + b][0], case.refs[b])).max() <= 1e-12
            else:
                assert (got['bleu'][b, w] == 0.0).all()
    if weights == 'default':
        assert got['reward'][0, 0] < 1e-6                                        # the empty rollout
        n = min(4, len(case.refs[1][0].split()))                                  # equal to the only reference: a cosine
        assert abs(got['cider'][1, 0] - 10.0 * n / 4) <= 1e-9 and abs(got['bleu'][1, 0, 0] - 1.0) <= 1e-6      # of 1 per order
        # the leave-one-out baseline on the same rewards
        loo = rr.score_ids(case.ids, ref_ids, vocab, df_ids, REF_LEN, w_c, w_b, rr.LEAVE_ONE_OUT)
        r = loo['reward']
        for b in range(B):
            for w in range(W):
                assert abs(loo['baseline'][b, w] - (r[b].sum() - r[b, w]) / (W - 1)) <= 1e-12
        assert np.abs(loo['advantage'].sum(axis=0)).max() <= 1e-5 * max(1.0, np.abs(r).max())


@pytest.mark.parametrize('shape', CASES)
def test_reference_equals_the_native_host_scorer(shape):
    try:
        L.load()
    except L.ComicHipError as e:
        pytest.skip('the library is not built: %s' % e)
    from comic_amd.scst.scorers import captionScorer
    case = make_case(*shape)
    w_c, w_b = WEIGHTS['default']
    vocab, ref_ids, df_ids = on_ids(case)
    got = rr.score_ids(case.ids, ref_ids, vocab, df_ids, REF_LEN, w_c, w_b, rr.ROW, case.base_ids)
    T, B, W = case.ids.shape
    sample = [[s] for s in text_rows(case, case.ids.transpose(2, 1, 0).reshape(W * B, T))]
    greedy = [[s] for s in text_rows(case, case.base_ids.T)]
    scorer = captionScorer(case.df, dict(ciderD=w_c, bleu=list(w_b)), n_threads=2)
    _, sc_sample, sc_greedy = scorer.get_hypo_scores(case.refs, sample, greedy)
    assert np.abs(got['reward'][:, :W].T.reshape(-1) - sc_sample).max() <= 1e-12
    assert np.abs(np.tile(got['reward'][:, W], W) - sc_greedy).max() <= 1e-12
    assert np.abs(scorer.get_scores(case.refs, sample) - sc_sample).max() == 0.0


@pytest.mark.parametrize('shape', CASES)
def test_canonical_words_are_the_words_of_the_text(shape):
    case = make_case(*shape)
    vocab = RewardVocab(case.cfg)
    T, B, W = case.ids.shape
    odd = over = after = 0
    for b in range(B):
        for w in range(W):
            row = case.ids[:, b, w]
            words = rr.canonical_words(row, vocab.token_type, vocab.end_id, vocab.n_ids, vocab.radix_base, vocab.word_len)
            assert ' '.join(case.cfg.itow[str(i)] for i in words) == text_rows(case, row[None])[0]
            if vocab.token_type == 'radix':
                digits = [t for t in row if 0 <= t < vocab.radix_base]
                odd += len(digits) % vocab.word_len != 0
                over += len(words) < (len(digits) - (1 if len(digits) % vocab.word_len else 0) + vocab.word_len - 1) // vocab.word_len
            first = np.flatnonzero(row == vocab.end_id)
            after += bool(len(first)) and bool((row[first[0]:] != vocab.end_id).any())
    assert after > 0                                             # tokens after the first <EOS>
    if vocab.token_type == 'radix':
        assert odd > 0 and over > 0                              # an odd digit count; a word id >= the vocabulary


def test_canonical_words_by_hand():
    cw = rr.canonical_words
    assert cw([3, 10, 4, -1, 5, 10, 11, 12], 'word', 10, 11) == [3, 4, 5]
    assert cw([1, 2, 3, 0, 5, 4, 1], 'radix', 5, 11, 4, 2) == [6]                      # 12 | 30 -> 6, 12 dropped; 1 dropped
    assert cw([2, 3, 0, 1], 'radix', 5, 11, 4, 2) == [1]                               # 23 = 11: the id the table lacks
    assert cw([0, 0, 1, 0, 1, 2, 2, 0], 'radix', 4, 12, 3, 3) == [1, 5, 2]             # 001 | 012 | 2(0 dropped): short group
    assert cw([0, 0, 1, 0, 1, 2, 2], 'radix', 4, 12, 3, 3) == [1, 5]                   # 7 digits: one dropped, no short group
    assert cw([], 'word', 10, 11) == [] and cw([4, 4], 'radix', 5, 11, 4, 2) == []


def test_keys_are_the_table_builders():
    toks = np.array([[5], [300]]), np.array([[5, 6, 7], [1, 0, 300]])
    for t in toks:
        assert cdec.ngram_keys(t).tolist() == [rr.ngram_key(x) for x in t.tolist()]


# ---- the vocabulary, the packer, the table ----------------------------------------------------------------------------------
def test_vocabulary_and_packer():
    cfg = make_config('radix4')
    v = RewardVocab(cfg)
    assert (v.size, v.n_ids, v.word_len, v.radix_base, v.end_id, v.token_type) == (12, 11, 2, 4, 5, 'radix')
    w = RewardVocab(make_config('word'))
    assert (w.n_ids, w.word_len, w.end_id) == (11, 1, 10)
    assert v.id('a') == 0 and v.id('<EOS>') == 10 and v.id('zebra') == 12 and v.id('yak') == 13 and v.id('zebra') == 12
    assert v.id('<PAD>') == 14                                   # no word id: an extended one, never the padding
    packed = RewardRefs.pack([['a zebra b', 'c'], ['yak']], v)
    assert packed.refs.dtype == np.int32 and packed.refs.shape == (2, 2, 3) and packed.n_refs.tolist() == [2, 1]
    assert packed.refs.tolist() == [[[0, 12, 1], [2, -1, -1]], [[13, -1, -1], [-1, -1, -1]]]
    for bad, field in (([['a'] * 9], 'references'), ([[' '.join(['a'] * 65)]], 'words'), ([['a'], []], 'reference'), ([], 'reference')):
        with pytest.raises(ValueError, match=field):
            RewardRefs.pack(bad, v)
    assert RewardRefs.pack([['']], v).refs.shape == (1, 1, 1)
    with pytest.raises(ValueError, match='char'):
        RewardVocab(SimpleNamespace(token_type='char', radix_base=0, wtoi={}))
    spaced = make_config('word')
    spaced.wtoi['two words'] = 11
    with pytest.raises(ValueError, match='white space'):
        RewardVocab(spaced)


def test_reward_from_pickle_keeps_every_ngram():
    case = make_case('word', 12, 7, 5, 5)
    r = Reward.from_pickle(case.df, case.cfg, baseline='mean', weights_ciderD=1.0, weights_bleu=(0, 0, 0, 2))
    df = case.df['document_frequency']
    assert r.idf.stride == 1 and r.idf.kept == len(df) and r.idf.skipped == 0
    assert any('zebra' in ng for ng in df) and any('<EOS>' in ng for ng in df)
    from tests import consensus_ref as cr
    for ng, cnt in df.items():
        key = rr.ngram_key([r.vocab.id(w) for w in ng])
        assert cr.table_lookup((r.idf.keys, r.idf.g), key, None) == np.log(float(REF_LEN)) - np.log(max(1.0, cnt))
    # the consensus table's builder is unchanged: the special words are still left out of it
    enc = {w: [i] for w, i in case.cfg.wtoi.items()}
    assert NgramIdf.from_document_frequency(df, REF_LEN, enc, 1).skipped > 0


# ---- Reward ------------------------------------------------------------------------------------------------------------------
def test_reward_identity_and_check():
    v = RewardVocab(make_config('word'))
    a, b = Reward(1.0, (0, 0, 0, 2), None, 'mean', v), Reward(1, [0, 0, 0, 2.0], None, 'mean', v)
    assert a == b and hash(a) == hash(b) and a != Reward(1.0, (0, 0, 0, 2), None, 'greedy', v)
    assert len({a, b, Reward(2.0, (0, 0, 0, 2), None, 'mean', v)}) == 2
    a.check(32, 64)
    Reward(vocab=v, baseline='greedy').check(7, 20, 20)
    Reward(vocab=RewardVocab(make_config('radix3')), baseline='none').check(1, 192)


@pytest.mark.parametrize('kw,beam,steps,base,field', [
    (dict(), 33, 20, 20, 'beam'),
    (dict(), 0, 20, 20, 'beam'),
    (dict(), 5, 65, 20, 'max_steps'),
    (dict(), 5, 20, 65, 'baseline_ids'),
    (dict(), 5, 20, None, 'baseline_ids'),
    (dict(baseline='mean'), 1, 20, None, 'beam'),
    (dict(baseline='median'), 5, 20, None, 'baseline'),
    (dict(weights_bleu=(0, 0, 1)), 5, 20, 20, 'weights_bleu'),
    (dict(weights_ciderD=float('nan')), 5, 20, 20, 'weights'),
    (dict(sigma=0.0), 5, 20, 20, 'sigma'),
    (dict(idf=NgramIdf(np.zeros(2, np.uint64), np.zeros(2), 1.0, 2)), 5, 20, 20, 'idf'),
    (dict(vocab=None), 5, 20, 20, 'vocab'),
])
def test_reward_check_refuses(kw, beam, steps, base, field):
    args = dict(vocab=RewardVocab(make_config('word')))
    args.update(kw)
    with pytest.raises(ValueError, match=field):
        Reward(**args).check(beam, steps, base)


def test_the_c_entries_refuse_before_any_launch():
    """(No GPU is needed: every one of these returns before the launch.)"""
    lib = L.load()
    ws = lib.comic_scst_reward_workspace
    assert ws(32, 7, 1, 20, 20, 1, 5, 20) > 0 and ws(2, 32, 0, 16, 0, 1, 5, 16) > 0
    small, large = ws(1, 2, 0, 8, 0, 1, 1, 8), ws(1, 4, 0, 8, 0, 1, 2, 8)
    assert large - small == 3 * 8 * 72                           # 72 bytes a word, caption by caption
    assert ws(1, 32, 1, 64, 64, 1, 8, 64) == -1                  # 41 captions of 64 words: beyond the LDS
    assert 'LDS' in lib.comic_last_error().decode()
    for args in ((1, 33, 0, 8, 0, 1, 1, 8), (1, 0, 0, 8, 0, 1, 1, 8), (1, 2, 0, 65, 0, 1, 1, 8), (1, 2, 0, 8, 0, 1, 9, 8),
                 (1, 2, 0, 8, 0, 1, 1, 65), (1, 2, 0, 8, 0, 9, 1, 8), (1, 2, 1, 8, 0, 1, 1, 8), (0, 2, 0, 8, 0, 1, 1, 8)):
        assert ws(*args) == -1, args
    wb = (L.C.c_double * 4)(0, 0, 0, 2)
    rc = lib.comic_scst_reward(None, 65, 2, 5, None, 0, None, 0, 1, 0, 1, 12, None, None, 1, 8, None, None, 0, 0.0, 6.0, 1.0, wb, 0,
                               None, None, None, None, None, None)
    assert rc == 2 and 'T = 65' in lib.comic_last_error().decode()
    rc = lib.comic_scst_reward(None, 8, 2, 1, None, 0, None, 0, 1, 0, 1, 12, None, None, 1, 8, None, None, 0, 0.0, 6.0, 1.0, wb, 2,
                               None, None, None, None, None, None)
    assert rc == 2                                                # NULL pointers are refused first; W = 1 never launches
    assert lib.comic_scst_coefficients(None, None, 0, 5, None, None, None) == 2


def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS
        assert re.search(r'\b%s\(' % name, header), name
    assert '#define COMIC_ABI_VERSION 1' in header               # additive change
    m = re.search(r'\bcomic_scst_reward_workspace\(', header)
    doc = header[max(0, m.start() - 6000):m.start()]
    for word in ('common/scst/scorers.py:43-171', 'W <= 32', 'R <= 8', 'LEAVE_ONE_OUT', 'hypothesis-major', '1e-12f'):
        assert word in doc, word
    src = os.path.join(ROOT, 'comic-compact-image-captioning-with-attention_amd', 'csrc')
    for f in ('consensus.hip', 'scst_reward.hip'):
        assert '#include "ngram_dev.h"' in open(os.path.join(src, f)).read()
    assert ' scst_reward.hip ' in open(os.path.join(src, 'Makefile')).read()


# ---- the host forms of the baseline and the coefficients -------------------------------------------------------------------
def test_leave_one_out_on_the_host():
    from comic_amd.train_fn import leave_one_out
    sc = np.arange(12, dtype=np.float64) ** 1.5                   # W = 3, B = 4, hypothesis-major
    adv, base = leave_one_out(sc, 3)
    m = sc.reshape(3, 4)
    for w in range(3):
        for b in range(4):
            assert abs(base[w * 4 + b] - (m[:, b].sum() - m[w, b]) / 2) <= 1e-12
    assert np.abs(adv.reshape(3, 4).sum(axis=0)).max() <= 1e-12 and adv.shape == (12,)


def test_coefficients_formula():
    wm = np.array([[1, 1, 1, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]], np.float32)
    coef, rs = rr.coefficients(wm, [0.5, -2.0, 3.0])
    assert coef.dtype == rs.dtype == np.float32 and coef.shape == rs.shape == (3, 5)
    assert np.allclose(coef[0], [0.5 / 3 / 3] * 3 + [0, 0], rtol=1e-6) and (coef[1] == 0).all()
    assert np.allclose(rs[2], 3.0 / 3 / 5, rtol=1e-6) and rs[1, 0] == np.float32(np.float32(-2.0) / np.float32(3)) / np.float32(1e-12)


# ---- the flags ----------------------------------------------------------------------------------------------------------------
def _train_cli():
    spec = importlib.util.spec_from_file_location('cli_train_scst_flags', os.path.join(ROOT, 'src', 'train.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flags_defaults_refusals_and_directory_names(tmp_path):
    cli = _train_cli()
    parser = cli.create_parser()
    d = parser.parse_args([])
    assert (d.scst_rollout, d.scst_temperature, d.scst_baseline, d.scst_reward) == ('beam', 1.0, 'greedy', 'host')
    assert cli.scst_dir_suffix(d) == ''
    for bad in (['--scst_rollout', 'greedy'], ['--scst_baseline', 'median'], ['--scst_reward', 'gpu']):
        with pytest.raises(SystemExit):
            parser.parse_args(bad)
    sfx = lambda *a: cli.scst_dir_suffix(parser.parse_args(list(a)))
    assert sfx('--scst_rollout', 'sample') == '_smp'
    assert sfx('--scst_rollout', 'sample', '--scst_temperature', '0.7') == '_smp_t0.7'
    assert sfx('--scst_baseline', 'mean') == '_loo'
    assert sfx('--scst_rollout', 'sample', '--scst_baseline', 'mean', '--scst_reward', 'device') == '_smp_loo'
    assert sfx('--scst_reward', 'device') == '' and sfx('--scst_temperature', '0.7') == ''
    # the run directory and the configuration
    base = ['--log_root', str(tmp_path), '--train_mode', 'scst', '--token_type', 'word', '--scst_beam_size', '3']
    name = 'word_add_LN_softmax_h8_tie_lstm'
    os.makedirs(os.path.join(str(tmp_path), 'mscoco', name + '_cnnFT_run_01'))
    kw, fn, _ = cli.build_kwargs(parser.parse_args(base))
    assert os.path.basename(kw['log_path']) == name + '_cnnFT_SCST_beam_3_CrD_1.0_B1_0.0_B4_2.0_run_01'
    assert (kw['scst_rollout'], kw['scst_temperature'], kw['scst_baseline'], kw['scst_reward']) == ('beam', 1.0, 'greedy', 'host')
    kw, fn, _ = cli.build_kwargs(parser.parse_args(base + ['--scst_rollout', 'sample', '--scst_temperature', '0.5',
                                                            '--scst_baseline', 'mean', '--scst_reward', 'device']))
    assert os.path.basename(kw['log_path']) == name + '_cnnFT_SCST_beam_3_CrD_1.0_B1_0.0_B4_2.0_smp_t0.5_loo_run_01'
    assert fn == 'train_fn_scst' and kw['scst_reward'] == 'device' and kw['scst_temperature'] == 0.5
    with pytest.raises(ValueError, match='scst_beam_size'):
        cli.build_kwargs(parser.parse_args(base[:-1] + ['1', '--scst_baseline', 'mean']))
    for one in (['--scst_reward', 'device'], ['--scst_rollout', 'sample']):      # one rollout decodes through another path
        with pytest.raises(ValueError, match='scst_beam_size'):
            cli.build_kwargs(parser.parse_args(base[:-1] + ['1'] + one))
    with pytest.raises(ValueError, match='char'):
        cli.refuse_bad_scst_options(dict(train_mode='scst', scst_reward='device', token_type='char'))
    with pytest.raises(ValueError, match='scst_temperature'):
        cli.refuse_bad_scst_options(dict(train_mode='scst', scst_rollout='sample', scst_temperature=0.0))
    cli.refuse_bad_scst_options(dict(train_mode='decoder', scst_reward='device', token_type='char'))   # not an SCST run
    from comic_amd.train_fn import scst_options
    o = scst_options(SimpleNamespace())                          # a configuration from before the flags
    assert (o.rollout, o.temperature, o.baseline, o.reward, o.default) == ('beam', 1.0, 'greedy', 'host', True)
    assert not scst_options(SimpleNamespace(scst_reward='device')).default
