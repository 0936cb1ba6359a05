"""Beam search with required words, the host side (no GPU): the rule of tests/beam_required_ref.py on hand-worked histories,
the dead-slot fill of the banked selection, BeamRequired.check and required_from_config, and the property that ties the
reference loop to the rule -- every finite slot of bank c holds a history of progress c."""
import json
import types

import numpy as np
import pytest

from comic_amd import decoder as cdec
from comic_amd.decoder import BeamConstraints, BeamGroups, BeamRequired, BeamSampling
from tests import beam_required_ref as rref


def _special(*pairs):
    out = np.zeros((4, 2), np.int32)
    out[:, 0] = -1
    for q, (tok, dest) in pairs:
        out[q] = (tok, dest)
    return out


def _table(h, req, S):
    base, special = rref.base_and_specials(h, np.asarray(req), S)
    return base, special.tolist()


# ------------------------------------------------------------------ hand-worked histories ---------------------------------
def test_one_token_per_word_counts_the_words_present():
    req = [[5], [7], [9]]
    assert [rref.progress(h, req, 1) for h in ([], [1], [5], [5, 5], [7, 1, 5], [9, 7, 5])] == [0, 0, 1, 1, 2, 3]
    assert _table([], req, 1) == (0, _special((0, (5, 1)), (1, (7, 1)), (2, (9, 1))).tolist())
    assert _table([7, 1], req, 1) == (1, _special((0, (5, 2)), (2, (9, 2))).tolist())
    assert _table([9, 7, 5], req, 1) == (3, _special().tolist())


def test_two_tokens_per_word_mid_word_and_at_boundaries():
    req = [[5, 6], [7, 8]]
    # at a word boundary (k = 0): the first token of every unmet word leads one bank up
    assert rref.progress([], req, 2) == 0
    assert _table([], req, 2) == (0, _special((0, (5, 1)), (1, (7, 1))).tolist())
    # mid-word with a partial (k = 1): the bank is S*m + 1, the base S*m, and only the word's next token completes it
    assert rref.progress([5], req, 2) == 1
    assert _table([5], req, 2) == (0, _special((0, (6, 2))).tolist())
    # the word completed: a boundary again, one word met
    assert rref.progress([5, 6], req, 2) == 2
    assert _table([5, 6], req, 2) == (2, _special((1, (7, 3))).tolist())
    assert rref.progress([5, 6, 7], req, 2) == 3
    assert _table([5, 6, 7], req, 2) == (2, _special((1, (8, 4))).tolist())
    assert rref.progress([5, 6, 7, 8], req, 2) == 4
    # an unaligned match is none: [1, 5, 6, 1] holds 5 6 at i = 1
    assert rref.progress([1, 5, 6, 1], req, 2) == 0


def test_a_lost_partial_falls_back_to_the_base():
    req = [[5, 6], [7, 8]]
    assert rref.progress([5, 6, 7], req, 2) == 3
    assert rref.progress([5, 6, 7, 1], req, 2) == 2               # the partial of word 1 is lost, word 0 stays met
    assert rref.progress([5, 1], req, 2) == 0
    # mid-word without a partial: no special at all, every token leads to the base
    assert _table([1], req, 2) == (0, _special().tolist())
    assert _table([5, 6, 1], req, 2) == (2, _special().tolist())


def test_two_words_sharing_a_prefix_and_a_word_required_twice():
    req = [[5, 6], [5, 8]]
    assert _table([], req, 2) == (0, _special((0, (5, 1)), (1, (5, 1))).tolist())      # the same token, the same dest
    assert _table([5], req, 2) == (0, _special((0, (6, 2)), (1, (8, 2))).tolist())
    assert rref.progress([5, 6, 5], req, 2) == 3
    twice = [[5, 6], [5, 6]]                                       # one emission completes both: gain 2
    assert _table([5], twice, 2) == (0, _special((0, (6, 4)), (1, (6, 4))).tolist())
    assert rref.progress([5, 6], twice, 2) == 4
    assert _table([], [[5], [5]], 1) == (0, _special((0, (5, 2)), (1, (5, 2))).tolist())


def test_padding_rows_and_an_all_padding_image():
    req = [[5, 6], [-1, -1]]
    assert rref.progress([], req, 2) == 2 and rref.progress([5], req, 2) == 3 and rref.progress([5, 6], req, 2) == 4
    assert _table([], req, 2) == (2, _special((0, (5, 3))).tolist())
    none = [[-1], [-1], [-1]]
    assert rref.progress([], none, 1) == 3 and rref.progress([4, 4], none, 1) == 3
    assert _table([4], none, 1) == (3, _special().tolist())
    lp, fin, ln = rref.init_state(np.array([req, [[5, 6], [7, 8]], [[-1, -1], [-1, -1]]]), 10, 2)
    assert np.argmax(fin == 0, axis=1).tolist() == [4, 0, 8] and (fin.sum(axis=1) == 9).all()
    assert (lp[fin == 0] == 0).all() and np.isneginf(lp[fin == 1]).all() and (ln == 0).all()


def test_the_table_is_the_progress_of_every_extension():
    """dest(v) read off the table == progress(h ++ v) for every token, over random histories, words and paddings."""
    rng = np.random.default_rng(0)
    V = 7
    for S in (1, 2, 3, 4):
        for C in (1, 2, 3, 4):
            for _ in range(150):
                req = rng.integers(0, V - 1, (C, S))
                if rng.random() < 0.3:
                    req[rng.integers(0, C)] = -1
                h = rng.integers(0, V - 1, rng.integers(0, 9)).tolist()
                base, special = rref.base_and_specials(h, req, S)
                assert 0 <= base <= rref.progress(h, req, S) <= C * S
                dest = rref.table_dest(np.array([[base]]), special[None, None], np.zeros((1, 1), int), V, C * S + 1)[0, 0]
                assert dest.tolist() == [rref.progress(h + [v], req, S) for v in range(V)], (h, req.tolist())


# ------------------------------------------------------------------ the banked selection ----------------------------------
def test_a_short_bank_is_filled_with_dead_slots():
    """W = 6 in three banks of two.  Bank 2 has ONE eligible candidate (the special of row 0), bank 1 the finished row 2's
    candidates and row 1's special, bank 0 everything else."""
    B, W, V, end_id = 1, 6, 9, 8
    lp = np.log(np.full((B, W, V), 1.0 / V))
    lp[0, 0, 3] += 1.0
    lp[0, 1, 4] += 2.0
    log_probs = np.array([[-1.0, -2.0, -0.5, -np.inf, -np.inf, -np.inf]])
    finished = np.array([[0, 0, 1, 1, 1, 1]], np.int32)
    lengths = np.array([[2, 3, 4, 0, 0, 7]], np.int64)
    base = np.zeros((B, W), np.int32)
    special = np.zeros((B, W, 4, 2), np.int32)
    special[..., 0] = -1
    special[0, 0, 0] = (3, 2)
    special[0, 1, 2] = (4, 1)
    r = rref.ref_select_banks(lp, log_probs, finished, lengths, end_id, 0.0, base, special, 3)
    assert r['eligible'].tolist() == [[2 * V - 2, V + 1, 1]]
    # bank 0: rows 0 and 1 minus their specials; bank 1: the finished row's <EOS> (-0.5), then row 1's special
    assert r['parent'][0].tolist() == [0, 0, 2, 1, 0, 5]
    assert r['word'][0, 2:].tolist() == [end_id, 4, 3, end_id]
    assert r['finished'][0].tolist() == [0, 0, 1, 0, 0, 1]
    assert r['lengths'][0].tolist() == [3, 3, 4, 4, 3, 7]         # the dead slot 5 keeps ITS OWN previous length
    assert np.isneginf(r['scores'][0, 5]) and np.isneginf(r['log_probs'][0, 5]) and np.isfinite(r['scores'][0, :5]).all()
    assert r['scores'][0, 2] == -0.5 and np.isclose(r['scores'][0, 4], -1.0 + lp[0, 0, 3])
    # a banned special (-inf) is not eligible: the bank stays empty, both slots dead
    lp[0, 0, 3] = -np.inf
    r = rref.ref_select_banks(lp, log_probs, finished, lengths, end_id, 0.0, base, special, 3)
    assert r['eligible'][0, 2] == 0 and r['parent'][0, 4:].tolist() == [4, 5] and r['finished'][0, 4:].tolist() == [1, 1]
    assert r['lengths'][0, 4:].tolist() == [0, 7] and np.isneginf(r['scores'][0, 4:]).all()
    assert rref.result_rule(r['scores'], 3, 1)[0].tolist() == [2]


def test_the_result_rule_takes_the_highest_bank_that_holds_a_caption():
    sc = np.array([[-1, -2, -3, -4, -np.inf, -np.inf], [-1, -2, -np.inf, -np.inf, -5, -np.inf],
                   [-np.inf] * 6], np.float32)
    rq = BeamRequired(np.zeros((3, 2, 1), np.int32))
    for best, met in (rq.result(sc), rref.result_rule(sc, 3, 1)):
        assert best.tolist() == [2, 4, 0] and met.tolist() == [1, 2, 0]
    best, met = BeamRequired(np.zeros((3, 1, 2), np.int32)).result(sc)
    assert best.tolist() == [2, 4, 0] and met.tolist() == [0, 1, 0]


def test_every_finite_slot_of_a_bank_has_that_progress():
    """The reference loop on a random step distribution (no decoder): after every step, the history of every slot with a
    finite log-probability has the progress of its bank -- the table and the selection agree with the rule."""
    rng = np.random.default_rng(4)
    for C, S, W in ((2, 1, 6), (2, 2, 10), (3, 1, 8), (1, 3, 4)):
        B, V = 3, 12
        banks = C * S + 1
        Wb = W // banks
        req = rng.integers(0, V - 1, (B, C, S)).astype(np.int32)
        req[0, C - 1] = -1
        log_probs, finished, lengths = rref.init_state(req, W, S)
        log_probs = log_probs.astype(np.float64)
        hists = [[] for _ in range(B * W)]
        seen = set()
        for t in range(9):
            logits = rng.standard_normal((B, W, V)) * 2
            lp = logits - np.log(np.exp(logits).sum(axis=-1, keepdims=True))
            base, special = rref.table_of(hists, req, S, W)
            r = rref.ref_select_banks(lp, log_probs, finished, lengths, V - 1, 0.0, base, special, banks)
            gidx = (np.arange(B)[:, None] * W + r['parent']).reshape(-1)
            fin_before = np.asarray(finished).reshape(-1)[gidx]
            # (a finished beam emits <EOS> for ever: its progress is that of the tokens before)
            hists = [hists[g] + ([] if f else [int(w)]) for g, w, f in zip(gidx, r['word'].reshape(-1), fin_before)]
            log_probs, finished, lengths = r['log_probs'], r['finished'], r['lengths']
            for i, h in enumerate(hists):
                if np.isfinite(log_probs.reshape(-1)[i]):
                    body = h[:h.index(V - 1)] if V - 1 in h else h
                    assert rref.progress(body, req[i // W], S) == (i % W) // Wb, (C, S, t, i, h)
                    seen.add((i % W) // Wb)
        assert seen == set(range(banks))


# ------------------------------------------------------------------ BeamRequired -------------------------------------------
def _spec(V=258, end_id=257):
    return types.SimpleNamespace(V=V, end_id=end_id)


def test_beam_required_is_hashed_by_its_shape_only():
    a, b = BeamRequired(np.zeros((3, 2, 1), np.int32)), BeamRequired(np.ones((5, 2, 1), np.int32))
    assert a == b and hash(a) == hash(b) and a.ctx_key() == ('required', 2, 1) and a.banks == 3
    assert a != BeamRequired(np.zeros((3, 1, 2), np.int32))
    with pytest.raises(ValueError, match='ids must be'):
        BeamRequired(np.zeros((3, 2), np.int32))


def test_check_refuses_on_the_host():
    ok = np.array([[[5], [6]], [[7], [-1]]], np.int32)
    BeamRequired(ok).check(_spec(), 6, 2, 14, BeamConstraints(min_length=3), BeamGroups(1, 0.0), BeamSampling(enabled=False))
    for ids, kw, beam, what in (
            (ok, {}, 4, r'3 banks \(n_words 2 \* stride 1 \+ 1\) do not divide the beam width 4'),
            (np.zeros((2, 5, 1)), {}, 6, 'n_words must be in'), (np.zeros((2, 1, 5)), {}, 6, 'stride must be in'),
            (np.array([[[257]], [[3]]]), {}, 6, 'end_id 257 cannot be required'),
            (np.array([[[258]], [[3]]]), {}, 6, 'token 258 is outside the vocabulary of 258'),
            (np.array([[[5, -1]], [[3, 4]]]), {}, 6, 'all of its tokens or in none'),
            (ok, dict(batch=3), 6, 'the table holds 2 images, the batch 3'),
            (ok, dict(groups=BeamGroups(2, 0.5)), 6, 'do not combine with beam groups'),
            (ok, dict(sampling=BeamSampling()), 6, 'do not combine with sampling')):
        with pytest.raises(ValueError, match=what):
            BeamRequired(ids).check(_spec(), beam, **kw)
    with pytest.raises(ValueError, match=r'V = 24 is too small: beam 6 \+ 1 suppress \+ 1 \+ max_steps 14 \+ 4 required = 26'):
        BeamRequired(ok).check(_spec(24, 23), 6, 2, 14, BeamConstraints(min_length=2, suppress=(3,)))
    with pytest.raises(ValueError, match='exceeds 65536'):
        BeamRequired(ok).check(_spec(70000, 1), 6)


# ------------------------------------------------------------------ required_from_config ------------------------------------
def _config(tmp_path, table, **kw):
    path = tmp_path / 'tags.json'
    path.write_text(json.dumps(table))
    wtoi = {'<PAD>': -1, 'a': 0, 'dog': 1, 'cat': 2, 'bench': 3, '<UNK>': 4, '<GO>': 5, '<EOS>': 6}
    base = dict(infer_require_file=str(path), token_type='word', wtoi=wtoi, radix_base=2, infer_beam_size=6)
    base.update(kw)
    return types.SimpleNamespace(**base)


FILES = ['/data/images/COCO_test2014_000000000001.jpg', '/data/images/COCO_test2014_000000000002.jpg',
         '/data/images/COCO_test2014_000000000003.jpg']


def test_required_from_config_word_tokens(tmp_path, capsys):
    c = _config(tmp_path, {'1': ['dog', 'zebra', 'dog'], 'COCO_test2014_000000000002.jpg': ['cat', '<EOS>', 'bench']})
    assert cdec.required_from_config(types.SimpleNamespace(infer_beam_size=3)) is None
    assert cdec.required_dir_suffix(types.SimpleNamespace()) == ''
    c.infer_beam_size = 8
    assert cdec.required_from_config(c) == dict(n_words=3, stride=1, banks=4)
    r = cdec.required_from_config(c, FILES)
    assert (r['n_words'], r['stride'], r['banks']) == (3, 1, 4)
    assert r['required'].ids.tolist() == [[[1], [-1], [-1]], [[2], [3], [-1]], [[-1], [-1], [-1]]]
    assert r['words'] == [['dog'], ['cat', 'bench'], []] and r['dropped'] == [['zebra', 'dog'], ['<EOS>'], []]
    assert '2 of 3 images name words; 3 words kept, 3 dropped' in capsys.readouterr().out
    assert cdec.required_dir_suffix(c) == '_req3_tags'
    c.infer_require_words = 1
    c.infer_beam_size = 6
    r = cdec.required_from_config(c, FILES)
    assert r['required'].ids.tolist() == [[[1]], [[2]], [[-1]]] and r['dropped'][1] == ['<EOS>', 'bench']
    assert cdec.required_dir_suffix(c) == '_req1_tags'


def test_required_from_config_radix_tokens(tmp_path):
    # 8 entries in base 2: 4 digits per word; C = 2 -> 9 banks
    c = _config(tmp_path, {'3': ['bench', 'cat']}, token_type='radix', infer_beam_size=9)
    r = cdec.required_from_config(c, FILES)
    assert (r['n_words'], r['stride'], r['banks']) == (2, 4, 9)
    assert r['required'].ids[2].tolist() == [[0, 0, 1, 1], [0, 0, 1, 0]] and (r['required'].ids[:2] == -1).all()


def test_required_from_config_refusals(tmp_path):
    with pytest.raises(ValueError, match=r'infer_beam_size 6 is no multiple of 4 \(infer_require_words 3 \* 1 tokens'):
        cdec.required_from_config(_config(tmp_path, {'1': ['a', 'dog', 'cat']}))
    with pytest.raises(ValueError, match=r'infer_beam_size 10 is no multiple of 9 \(infer_require_words 2 \* 4 tokens'):
        cdec.required_from_config(_config(tmp_path, {'1': ['a', 'dog']}, token_type='radix', infer_beam_size=10))
    with pytest.raises(ValueError, match='not `char`'):
        cdec.required_from_config(_config(tmp_path, {'1': ['a']}, token_type='char'))
    with pytest.raises(ValueError, match='infer_require_words must be in'):
        cdec.required_from_config(_config(tmp_path, {'1': ['a']}, infer_require_words=5))
    with pytest.raises(ValueError, match='JSON object of image'):
        cdec.required_from_config(_config(tmp_path, ['a']))
