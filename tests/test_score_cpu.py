"""Caption scoring, the parts that need no GPU: the ABI declares and exports the entries, src/score.py parses its
arguments, tokenises a captions file and builds its output records."""
import importlib.util
import json
import math
import os
import re
import types

import numpy as np
import pytest

import comic_amd._lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('comic_decoder_score_workspace', 'comic_decoder_score', 'comic_decoder_score_path')


def _cli():
    spec = importlib.util.spec_from_file_location('cli_score', os.path.join(ROOT, 'src', 'score.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_declares_and_library_exports_the_score_entries():
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(comic_[a-z0-9_]+)\s*\(', header))
    lib = L.load()
    for name in ENTRIES:
        assert name in declared, name
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.comic_abi_version() == 1


def test_score_workspace_is_a_host_computation_and_smaller_than_training():
    """comic_decoder_score_workspace needs no device; at the word vocabulary it lacks the training step's d-logits block."""
    import ctypes as C
    from comic_amd import decoder as cdec
    spec = cdec.DecoderSpec(D=512, E=256, V=25599, C=2048, Cg=2048, H=8, M=25, token_type='word', start_id=25597, end_id=25598)
    d = spec.desc(False)
    lib = L.load()
    train, score = lib.comic_decoder_train_workspace(C.byref(d), 64, 20), lib.comic_decoder_score_workspace(C.byref(d), 64, 20)
    assert 0 < score < train - 64 * 20 * 25599 * 4, (train, score)
    assert lib.comic_decoder_score_workspace(C.byref(d), 0, 20) == -1


def test_score_cli_parses_its_arguments():
    cli = _cli()
    with pytest.raises(SystemExit):
        cli.create_parser().parse_args([])                    # --captions_file is required
    a = cli.create_parser().parse_args(['--captions_file', 'x/captions___5.json', '--infer_checkpoints', '5,7', '--cnn_dtype', 'f16',
                                        '--infer_set', 'valid', '--batch_size_infer', '4'])
    assert a.captions_file == 'x/captions___5.json' and a.cnn_dtype == 'f16' and a.infer_set == 'valid' and a.batch_size_infer == 4
    assert cli.find_checkpoints('.', a.infer_checkpoints) == ['5', '7']
    assert cli.create_parser().parse_args(['--captions_file', 'c.json']).cnn_dtype is None
    assert cli.image_id_of('val2014/COCO_val2014_000000000042.jpg') == 42


def test_score_cli_tokenises_and_builds_records_with_a_stubbed_scorer(tmp_path):
    cli = _cli()
    wtoi = {'<PAD>': -1, 'a': 0, 'cat': 1, 'dog': 2, 'sits': 3, '<UNK>': 4, '<GO>': 5, '<EOS>': 6}
    config = types.SimpleNamespace(token_type='word', wtoi=wtoi)
    entries = [dict(image_id=7, caption='a cat sits'), dict(image_id=9, caption='a dog'),
               dict(image_id=7, caption='a zebra')]           # an n-best list: image 7 twice; an unknown word
    path = tmp_path / 'captions___3.json'
    path.write_text(json.dumps(entries))
    entries = json.loads(path.read_text())
    ids = cli.tokenise([e['caption'] for e in entries], config)
    np.testing.assert_array_equal(ids, [[5, 0, 1, 3, 6], [5, 0, 2, 6, -1], [5, 0, 4, 6, -1]])
    filenames = ['val/COCO_val2014_000000000007.jpg', 'val/COCO_val2014_000000000009.jpg']
    images = np.arange(2, dtype=np.float32).reshape(2, 1)
    calls = []

    def scorer(imgs, ids):                  # log p = -0.5 per token, -1 more for the first image
        lens = (ids[:, 1:] >= 0).sum(axis=1)
        calls.append((imgs[:, 0].tolist(), ids.shape))
        return [-0.5 * n - (1.0 if im[0] == 0 else 0.0) for n, im in zip(lens, imgs)], lens
    records = cli.score_entries(entries, filenames, iter([(images, None)]), 2, config, scorer)
    assert calls == [([0.0, 1.0], (2, 5)), ([0.0], (1, 4))]          # round 0: both images; round 1: image 7's second caption
    want = [(7, 'a cat sits', -3.0, 4), (9, 'a dog', -1.5, 3), (7, 'a zebra', -2.5, 3)]
    for r, (iid, cap, lp, n) in zip(records, want):
        assert (r['image_id'], r['caption'], r['num_tokens']) == (iid, cap, n)
        assert r['log_prob'] == lp and r['perplexity'] == pytest.approx(math.exp(-lp / n), rel=1e-12)
    assert records[0]['perplexity'] == pytest.approx(math.exp(0.75)) and records[1]['perplexity'] == pytest.approx(math.exp(0.5))
    out = tmp_path / 'scores___3.json'
    out.write_text(json.dumps(records))
    assert json.loads(out.read_text()) == records            # the record round-trips through JSON
    with pytest.raises(ValueError):
        cli.score_entries(entries + [dict(image_id=11, caption='a')], filenames, iter([(images, None)]), 2, config, scorer)
