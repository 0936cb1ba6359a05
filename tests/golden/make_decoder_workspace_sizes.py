"""Generates tests/golden/decoder_workspace_sizes.json: what comic_decoder_train_workspace / _score_workspace /
_infer_workspace return (host computations, no device) for every geometry of tests/test_gpu_path.py's TRAIN_VARIANTS plus the
word vocabulary.  The committed file was written by the build BEFORE the workspace layouts got their single definitions in
csrc/decoder_exec.hip; tests/test_workspace_sizes_cpu.py pins every later build to it.  Run from the repo root:
python tests/golden/make_decoder_workspace_sizes.py"""
import ast
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from comic_amd import _lib as L, decoder as cdec  # noqa: E402

BASE = dict(D=128, E=64, V=258, C=192, Cg=192, H=8, M=25)          # tests/test_gpu_path.py: _spec_and_cfg
WORD = dict(D=512, E=256, V=25599, C=2048, Cg=2048, H=8, M=25, token_type='word', start_id=25597, end_id=25598)
BS, TS, ROWS, STEPS = (1, 6, 16, 23, 64, 80), (1, 11, 20, 29), (1, 50, 64, 65, 150), (0, 1, 20, 40)


def train_variants():
    tree = ast.parse(open(os.path.join(os.path.dirname(HERE), 'test_gpu_path.py')).read())
    node = next(n for n in tree.body if isinstance(n, ast.Assign) and n.targets[0].id == 'TRAIN_VARIANTS')
    return [{k.arg: ast.literal_eval(k.value) for k in e.keywords} for e in node.value.elts]      # a list of dict(...) calls


def sizes(kw):
    lib, d = L.load(), cdec.DecoderSpec(**kw).desc(False)
    d.flags = 0
    out = dict(spec=kw, train=[[lib.comic_decoder_train_workspace(C.byref(d), b, t) for t in TS] for b in BS],
               score=[[lib.comic_decoder_score_workspace(C.byref(d), b, t) for t in TS] for b in BS],
               infer=[[lib.comic_decoder_infer_workspace(C.byref(d), r, s) for s in STEPS] for r in ROWS])
    d.flags = L.DEC_NO_BEAM_LOGITS
    out['score_no_beam_logits'] = [[lib.comic_decoder_score_workspace(C.byref(d), b, t) for t in TS] for b in BS]
    return out


if __name__ == '__main__':
    doc = dict(B=BS, T=TS, rows=ROWS, max_steps=STEPS, cases=[sizes(dict(BASE, **kw)) for kw in train_variants()] + [sizes(WORD)])
    with open(os.path.join(HERE, 'decoder_workspace_sizes.json'), 'w') as f:
        f.write('{' + ',\n'.join('"%s": %s' % (k, json.dumps(doc[k])) for k in ('B', 'T', 'rows', 'max_steps')) + ',\n"cases": [\n'
                + ',\n'.join(json.dumps(c) for c in doc['cases']) + '\n]}\n')
    print('%d cases' % len(doc['cases']))
