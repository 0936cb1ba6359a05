"""Host side of ensemble beam search, no GPU: validation in decoder.EnsembleDecoder before anything touches the device, the
output file name, the infer.py flags, and the new entries in the header and the bindings."""
import importlib.util
import os
import re
from types import SimpleNamespace

import pytest

import comic_amd._lib as L
from comic_amd import decoder as cdec, infer_fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('comic_beam_step_ensemble_workspace', 'comic_beam_step_ensemble', 'comic_beam_step_ensemble_path',
               'comic_decoder_beam_ensemble_workspace', 'comic_decoder_beam_ensemble')


def _members(*specs):
    # stand-ins without parameters or a device: the constructor must refuse before it looks at either
    return [SimpleNamespace(spec=s) for s in specs]


def test_ensemble_refuses_mismatched_members_before_any_gpu_call():
    a = cdec.DecoderSpec()
    for other, field in ((cdec.DecoderSpec(V=300), 'V'), (cdec.DecoderSpec(end_id=255), 'end_id'),
                         (cdec.DecoderSpec(start_id=255), 'start_id'), (cdec.DecoderSpec(token_type='word'), 'token_type')):
        with pytest.raises(ValueError, match=field):
            cdec.EnsembleDecoder(_members(a, other))
    with pytest.raises(ValueError, match='1 to 8'):
        cdec.EnsembleDecoder(_members(*[a] * 9))
    with pytest.raises(ValueError, match='1 to 8'):
        cdec.EnsembleDecoder([])


@pytest.mark.parametrize('weights,what', [([0.5], 'weights for'), ([0.5, 0.6], 'sum to 1'), ([1.5, -0.5], '>= 0'),
                                          ([float('nan'), 1.0], '>= 0'), ([0.5, 0.5 + 1e-5], 'sum to 1')])
def test_ensemble_refuses_bad_weights(weights, what):
    a = cdec.DecoderSpec()
    with pytest.raises(ValueError, match=what):
        cdec.EnsembleDecoder(_members(a, a), weights)


def test_ensemble_weights_default_to_uniform_and_members_may_differ_in_geometry():
    a, b = cdec.DecoderSpec(), cdec.DecoderSpec(D=256, E=128, H=4, rnn_name='GRU', method='dot', C=832, M=196)
    assert cdec.check_ensemble([a, b, a]) == [1 / 3] * 3
    assert cdec.check_ensemble([a, b], [1, 0]) == [1.0, 0.0]
    assert cdec.check_ensemble([a, b], [0.25, 0.75 + 5e-7]) == [0.25, 0.75 + 5e-7]


def test_output_file_name():
    assert infer_fn.ensemble_name(['3', '7', '9']) == 'ens_3+7+9'
    assert 'captions___{}.json'.format(infer_fn.ensemble_name([12, 12])) == 'captions___ens_12+12.json'


def _infer_cli():
    spec = importlib.util.spec_from_file_location('cli_infer_flags', os.path.join(ROOT, 'src', 'infer.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_infer_flags_are_absent_by_default():
    """Flags left out do not reach the configuration (infer.py overlays only what is not None): without --infer_ensemble
    the per-checkpoint loop runs as before."""
    parser = _infer_cli().create_parser()
    overlay = {k: v for k, v in parser.parse_args([]).__dict__.items() if v is not None}
    assert 'infer_ensemble' not in overlay and 'infer_ensemble_weights' not in overlay
    assert overlay['infer_checkpoints'] == 'all' and overlay['infer_beam_size'] == 3
    args = parser.parse_args(['--infer_checkpoints', '3,7,9', '--infer_ensemble', '--infer_ensemble_weights', '0.5,0.3,0.2'])
    assert args.infer_ensemble is True and args.infer_ensemble_weights == '0.5,0.3,0.2'


def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS
        assert re.search(r'\b%s\(' % name, header), name
    assert 'ops_rnn.py:49-112' in header[header.index('comic_beam_step_ensemble_workspace') - 1500:]
    assert '#define COMIC_ABI_VERSION 1' in header               # additive change
