"""--cnn_dtype f16 on the host side (no GPU): CLI acceptance and refusal, the header's dtype code, tune-cache keys."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _train_module():
    spec = importlib.util.spec_from_file_location('cli_train_f16', os.path.join(ROOT, 'src', 'train.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_parser_accepts_f16():
    args = _train_module().create_parser().parse_args(['--cnn_dtype', 'f16'])
    assert args.cnn_dtype == 'f16'


def test_cnn_finetune_on_f16_is_refused_before_the_gpu():
    mod = _train_module()
    with pytest.raises(NotImplementedError, match='bf16 or bf16x3'):
        mod.check_supported({'train_mode': 'cnn_finetune', 'cnn_dtype': 'f16'})
    for mode in ('decoder', 'scst'):
        mod.check_supported({'train_mode': mode, 'cnn_dtype': 'f16'})
    mod.check_supported({'train_mode': 'cnn_finetune', 'cnn_dtype': 'bf16'})
    # main() refuses right after parsing: nothing is imported from torch, no directory is created
    with pytest.raises(NotImplementedError, match='forward-only'):
        mod.main(['--train_mode', 'cnn_finetune', '--cnn_dtype', 'f16', '--log_root', '/nonexistent/never/created'])
    assert not os.path.exists('/nonexistent/never/created')


def test_infer_parser_takes_an_optional_cnn_dtype():
    spec = importlib.util.spec_from_file_location('cli_infer_f16', os.path.join(ROOT, 'src', 'infer.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.create_parser().parse_args([]).cnn_dtype is None          # the training run's value applies
    assert mod.create_parser().parse_args(['--cnn_dtype', 'f16']).cnn_dtype == 'f16'


def test_header_defines_the_f16_dtype_code():
    h = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    assert re.search(r'^#define COMIC_F16 2$', h, re.M)
    assert re.search(r'^#define COMIC_BF16 1$', h, re.M) and re.search(r'^#define COMIC_ABI_VERSION 1$', h, re.M)
    assert 'comic_cnn_refresh_weights_dtype(' in h


def test_bf16_tune_keys_are_unchanged():
    from comic_amd import nets

    class P:
        name, pool_after_projection, fuse_pools, fuse_chains, x3 = 'inception_v3', True, True, True, False
        buffers, input, ops = [(224, 224, 3, True)], 0, [None] * 7

    def key(dtype, polite=0):
        e = nets.CnnEncoder.__new__(nets.CnnEncoder)
        e.plan, e.batch, e.dtype, e._polite_lds_kb = P, 64, dtype, polite
        return e._tune_key()

    assert key('bf16') == 'inception_v3:224x224:B64:par+fp+ch:7ops:polite0'
    assert key('f16') == key('bf16') + ':f16'
