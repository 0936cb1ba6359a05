"""The decoder executors' workspace sizes (comic_decoder_train_workspace / _score_workspace / _infer_workspace: host
computations) against tests/golden/decoder_workspace_sizes.json, entry by entry.  The file was recorded from the build in
which every size function restated its executor's block list by hand; each layout now has one definition in
csrc/decoder_exec.hip (TrainLayout, carve_infer) that both the size function and the executor run, and must give the same
bytes.  Regenerate only for a deliberate layout change: tests/golden/make_decoder_workspace_sizes.py."""
import ast
import ctypes as C
import json
import os

import pytest

import comic_amd._lib as L
from comic_amd import decoder as cdec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'decoder_workspace_sizes.json')))
BASE = dict(D=128, E=64, V=258, C=192, Cg=192, H=8, M=25)          # tests/test_gpu_path.py: _spec_and_cfg


def _train_variants():
    tree = ast.parse(open(os.path.join(ROOT, 'tests', 'test_gpu_path.py')).read())
    node = next(n for n in tree.body if isinstance(n, ast.Assign) and n.targets[0].id == 'TRAIN_VARIANTS')
    return [{k.arg: ast.literal_eval(k.value) for k in e.keywords} for e in node.value.elts]      # a list of dict(...) calls


def test_fixture_covers_every_train_variant_and_the_word_vocabulary():
    specs = [c['spec'] for c in GOLDEN['cases']]
    for kw in _train_variants():
        assert dict(BASE, **kw) in specs, kw
    assert any(s['V'] == 25599 for s in specs)
    assert {s.get('rnn_name', 'LSTM') for s in specs} == {'LSTM', 'LN_LSTM', 'GRU'}
    assert {s.get('init_method', 'first_input') for s in specs} == {'first_input', 'project_hidden'}
    assert {s.get('fm_projection', 'tied') for s in specs} == {None, 'tied', 'independent'}
    assert any(s.get('context_layer') for s in specs) and {s['M'] for s in specs} == {25, 64, 130, 196}
    assert (GOLDEN['B'], GOLDEN['T']) == ([1, 6, 16, 23, 64, 80], [1, 11, 20, 29])
    assert (GOLDEN['rows'], GOLDEN['max_steps']) == ([1, 50, 64, 65, 150], [0, 1, 20, 40])


@pytest.mark.parametrize('case', GOLDEN['cases'], ids=lambda c: '-'.join('%s=%s' % kv for kv in sorted(c['spec'].items())))
def test_workspace_sizes_equal_the_recorded_ones(case):
    lib, d = L.load(), cdec.DecoderSpec(**case['spec']).desc(False)
    for flags, key in ((0, 'score'), (L.DEC_NO_BEAM_LOGITS, 'score_no_beam_logits')):
        d.flags = flags
        for i, b in enumerate(GOLDEN['B']):
            for j, t in enumerate(GOLDEN['T']):
                assert lib.comic_decoder_score_workspace(C.byref(d), b, t) == case[key][i][j], (key, b, t)
                if not flags:
                    assert lib.comic_decoder_train_workspace(C.byref(d), b, t) == case['train'][i][j], ('train', b, t)
    for i, r in enumerate(GOLDEN['rows']):
        for j, s in enumerate(GOLDEN['max_steps']):
            assert lib.comic_decoder_infer_workspace(C.byref(d), r, s) == case['infer'][i][j], ('infer', r, s)
