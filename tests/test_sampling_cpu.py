"""Host side of sampling inside the beam step, no GPU: the generator of tests/beam_sampling_ref.py (range, exactness, a
frequency test), BeamSampling.check before anything touches the device, the struct, the new entries in the header and the
bindings, the infer.py flags and directory name, and the sampled-step reference itself on tiny hand-made inputs."""
import ctypes as C
import importlib.util
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import comic_amd._lib as L
from comic_amd import decoder as cdec
from comic_amd.decoder import BeamGroups, BeamSampling
from tests import beam_sampling_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('comic_beam_sample_noise', 'comic_beam_step_sampled_workspace', 'comic_beam_step_sampled',
               'comic_decoder_beam_sampled_workspace', 'comic_decoder_beam_sampled')


# ---- the generator ---------------------------------------------------------------------------------------------------------
def test_splitmix64_known_values():
    """The first outputs of the published splitmix64 stream seeded with 0 (state += golden gamma per draw) are
    splitmix64(0), splitmix64(gamma), ...: 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F."""
    gamma = 0x9E3779B97F4A7C15
    got = [int(sref.splitmix64(np.uint64((i * gamma) % 2 ** 64))[0]) for i in range(3)]
    assert got == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_noise_range_and_exactness():
    for seed, base, t in ((5, 0, 0), (2 ** 63 + 11, 1000, 7)):
        k, u, g = sref.noise(seed, base, 3, 64, t, 1000)
        assert k.min() >= 0 and k.max() < 2 ** 23
        assert (u.astype(np.float32).astype(np.float64) == u).all()           # exactly representable in fp32
        assert u.min() >= 2.0 ** -24 and u.max() <= 1 - 2.0 ** -24
        assert np.isfinite(g).all() and g.min() >= -2.82 and g.max() <= 16.64
    # the extremes of the draw
    lo, hi = -np.log(-np.log(2.0 ** -24)), -np.log(-np.log(1 - 2.0 ** -24))
    assert -2.82 < lo < -2.81 and 16.63 < hi < 16.64


def test_noise_is_keyed_by_the_image_not_by_the_batch():
    whole = sref.noise(5, 0, 4, 3, 2, 50)[0]
    np.testing.assert_array_equal(sref.noise(5, 2, 2, 3, 2, 50)[0], whole[2:])
    np.testing.assert_array_equal(sref.noise(5, 0, 2, 3, 2, 50)[0], whole[:2])
    assert not np.array_equal(sref.noise(6, 0, 4, 3, 2, 50)[0], whole)
    assert not np.array_equal(sref.noise(5, 0, 4, 3, 3, 50)[0], whole)
    assert len({tuple(whole[b, w]) for b in range(4) for w in range(3)}) == 12     # every (image, slot) its own stream


def test_frequencies_follow_the_distribution():
    """50 steps x 64 entries x 64 slots = 204 800 Gumbel-max draws from a fixed 12-way distribution.  Pearson's statistic
    against the 0.999 quantile of chi-square at 11 degrees of freedom, 31.26; computed on the CPU: 7.51."""
    logits = np.random.default_rng(1).standard_normal(12) * 1.5
    lp = logits - np.log(np.exp(logits).sum())
    counts = np.zeros(12)
    for t in range(50):
        g = sref.noise(9, 0, 64, 64, t, 12)[2]
        counts += np.bincount(np.argmax(lp[None, None, :] + g, axis=2).reshape(-1), minlength=12)
    assert counts.sum() == 204800
    expect = counts.sum() * np.exp(lp)
    stat = float(((counts - expect) ** 2 / expect).sum())
    print('Pearson statistic %.2f (bound 31.26)' % stat)
    assert stat < 31.26


# ---- BeamSampling ------------------------------------------------------------------------------------------------------------
def test_defaults_and_identity():
    s = BeamSampling()
    assert s.active and s.key() == (1.0, 0, True)
    assert not BeamSampling(enabled=False).active
    assert BeamSampling(0.7, 3) == BeamSampling('0.7', 3.0) and BeamSampling(0.7, 3) != BeamSampling(0.7, 4)
    assert len({BeamSampling(0.7, 3), BeamSampling(0.7, 3), BeamSampling(0.8, 3)}) == 2
    assert repr(BeamSampling(0.7, 3)) == 'BeamSampling(temperature=0.7, seed=3)'
    # a context is keyed by the temperature, not by the seed
    assert BeamSampling(0.7, 3).ctx_key() == BeamSampling(0.7, 4).ctx_key() != BeamSampling(0.8, 3).ctx_key()
    BeamSampling(0.7, 3).check(5)
    BeamSampling(0.7, 3).check(1)
    BeamSampling(0.7, 3).check(64, 0.0, BeamGroups(1, 0.5))
    np.testing.assert_array_equal(BeamSampling(0.7, 2 ** 64 - 1).seed_words(7).view(np.uint64), [2 ** 64 - 1, 7])


@pytest.mark.parametrize('kw,beam,lpw,groups,field', [
    (dict(temperature=0.0), 4, 0.0, None, 'temperature'),
    (dict(temperature=-1.0), 4, 0.0, None, 'temperature'),
    (dict(temperature=float('nan')), 4, 0.0, None, 'temperature'),
    (dict(temperature=float('inf')), 4, 0.0, None, 'temperature'),
    (dict(temperature=1e-39), 4, 0.0, None, 'reciprocal'),
    (dict(seed=-1), 4, 0.0, None, 'seed'),
    (dict(), 0, 0.0, None, 'number of samples'),
    (dict(), 65, 0.0, None, 'number of samples'),
    (dict(), 4, 0.7, None, 'length penalty'),
    (dict(), 4, 0.0, BeamGroups(2, 0.5), 'beam groups'),
])
def test_check_refuses(kw, beam, lpw, groups, field):
    with pytest.raises(ValueError, match=field):
        BeamSampling(**kw).check(beam, lpw, groups)


def test_struct_matches_the_header():
    assert C.sizeof(L.BeamSampling) == 16
    s = BeamSampling(0.5, 3).c_struct(0x1000)
    assert (s.temperature, s.seed_dev) == (0.5, 0x1000)
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    assert re.search(r'typedef struct comic_beam_sampling \{\s*float temperature;\s*const uint64_t\* seed_dev;\s*\} '
                     r'comic_beam_sampling;', header)


def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS
        m = re.search(r'\b%s\(' % name, header)
        assert m, name
        assert 'ops_rnn.py:49-112' in header[max(0, m.start() - 1500):m.start()], name
    assert '#define COMIC_ABI_VERSION 1' in header               # additive change
    lib = L.load()
    assert lib.comic_beam_step_sampled_workspace(0, 2, 3, 17) == -1
    # every slot's candidates carry their totals: B * chunks * W floats more than the ensemble step's workspace
    for n, B, W, V in ((2, 2, 5, 9001), (1, 50, 5, 25599), (1, 2, 3, 17)):
        chunks = max(1, min(min(32, 1024 // B), V // 1024))
        assert lib.comic_beam_step_sampled_workspace(n, B, W, V) \
            == lib.comic_beam_step_ensemble_workspace(n, B, W, V) + 4 * B * chunks * W


# ---- configuration and CLI ---------------------------------------------------------------------------------------------------
def _infer_cli():
    spec = importlib.util.spec_from_file_location('cli_infer_sample_flags', os.path.join(ROOT, 'src', 'infer.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_infer_flags_are_absent_by_default_and_parsed_when_given():
    parser = _infer_cli().create_parser()
    overlay = {k: v for k, v in parser.parse_args([]).__dict__.items() if v is not None}
    assert not {'infer_sample', 'infer_temperature', 'infer_sample_seed'} & set(overlay)
    args = parser.parse_args(['--infer_sample', '--infer_temperature', '0.7', '--infer_sample_seed', '3', '--infer_beam_size',
                              '5', '--infer_ensemble', '--infer_min_length', '4'])
    assert (args.infer_sample, args.infer_temperature, args.infer_sample_seed, args.infer_beam_size) == (True, 0.7, 3, 5)
    assert args.infer_ensemble is True and args.infer_min_length == 4


def test_sampling_from_config():
    ns = SimpleNamespace
    assert cdec.sampling_from_config(ns(infer_beam_size=5)) is None
    assert cdec.sampling_from_config(ns(infer_beam_size=5, infer_sample=None, infer_temperature=None,
                                        infer_sample_seed=None)) is None
    assert cdec.sampling_from_config(ns(infer_beam_size=5, infer_sample=True, infer_temperature=0.7, infer_sample_seed=3)) \
        == BeamSampling(0.7, 3)
    assert cdec.sampling_from_config(ns(infer_beam_size=5, infer_sample=True)) == BeamSampling(1.0, 0)
    assert not cdec.sampling_from_config(ns(infer_beam_size=5, infer_temperature=0.7)).active
    with pytest.raises(ValueError, match='temperature'):
        cdec.sampling_from_config(ns(infer_beam_size=5, infer_sample=True, infer_temperature=0.0))
    with pytest.raises(ValueError, match='beam groups'):
        cdec.sampling_from_config(ns(infer_beam_size=6, infer_sample=True, infer_beam_groups=3))
    with pytest.raises(ValueError, match='length penalty'):
        cdec.sampling_from_config(ns(infer_beam_size=5, infer_sample=True, infer_length_penalty_weight=0.7))
    assert cdec.sampling_from_config(ns(infer_beam_size=5, infer_sample=True, infer_beam_groups=1, infer_diversity=0.5,
                                        infer_length_penalty_weight=0.0)).active


def test_directory_suffix():
    parser = _infer_cli().create_parser()
    assert cdec.sampling_dir_suffix(parser.parse_args([])) == ''
    assert cdec.sampling_dir_suffix(parser.parse_args(['--infer_temperature', '0.7'])) == ''       # not sampling
    assert cdec.sampling_dir_suffix(parser.parse_args(['--infer_sample', '--infer_temperature', '0.7',
                                                       '--infer_sample_seed', '3'])) == '_smp_t0.7_s3'
    assert cdec.sampling_dir_suffix(parser.parse_args(['--infer_sample'])) == '_smp_t1_s0'
    both = parser.parse_args(['--infer_min_length', '8', '--infer_sample', '--infer_temperature', '0.25'])
    assert cdec.constraints_dir_suffix(both) + cdec.groups_dir_suffix(both) + cdec.sampling_dir_suffix(both) \
        == '_min8_ngram0_sup0_smp_t0.25_s0'


def test_sampled_radix_digits_that_spell_the_unmapped_word_id_are_skipped():
    """len(itow) counts '-1' (<PAD>), so word id len - 1 passes the `< vocab` filter without an entry: the strict decode
    raises as the reference's lookup does; the sampled path skips it like the ids >= vocab."""
    from comic_amd.ops import id_to_caption
    c = SimpleNamespace(token_type='radix', radix_base=256, itow={'-1': '<PAD>', '0': 'a', '1': 'b', '2': 'c'})
    ids = np.array([[0, 3, 2, 256], [1, 1, 257, 257]])
    with pytest.raises(KeyError, match='3'):
        id_to_caption(ids, c)
    assert id_to_caption(ids, c, skip_unmapped=True) == ['a c', 'b b']
    assert id_to_caption(ids[1:], c) == id_to_caption(ids[1:], c, skip_unmapped=True) == ['b b']
    wide = SimpleNamespace(token_type='radix', radix_base=2, itow={str(i): 'w%d' % i for i in range(-1, 8)})     # four digits
    assert id_to_caption(np.array([[0, 0, 1, 1, 0, 0, 0, 1, 0]]), wide, skip_unmapped=True) == ['w3 w1']
    with pytest.raises(KeyError, match='8'):
        id_to_caption(np.array([[1, 0, 0, 0]]), wide)
    assert id_to_caption(np.array([[1, 0, 0, 0, 0, 1, 1, 1]]), wide, skip_unmapped=True) == ['w7']


class _Stop(Exception):
    pass


def test_none_and_inactive_sampling_leave_the_call_path_alone():
    """Decoder.beam_search with sampling=None or an inactive BeamSampling must not route through the one-member ensemble;
    an active one does, with the sampling and the image base handed on.  (No GPU: the first device-touching call of
    either path is replaced.)"""
    dec = object.__new__(cdec.Decoder)
    dec.spec = SimpleNamespace(V=258)
    dec.torch = None
    seen = {}

    def infer_ctx(*a, **k):
        raise _Stop('plain')
    dec._infer_ctx = infer_ctx
    fm = SimpleNamespace(shape=(2, 25, 192))
    for smp in (None, BeamSampling(0.7, 3, enabled=False)):
        with pytest.raises(_Stop, match='plain'):
            dec.beam_search(fm, None, 4, 14, sampling=smp, image_base=9)
        assert '_self_ensemble' not in dec.__dict__

    class Ens:
        def _decode(self, *a):
            seen['options'] = a[-1]
            raise _Stop('ensemble')
    dec._self_ensemble = Ens()
    with pytest.raises(_Stop, match='ensemble'):
        dec.beam_search(fm, None, 4, 14, sampling=BeamSampling(0.7, 3), image_base=9)
    assert seen['options'].sampling == BeamSampling(0.7, 3) and seen['options'].image_base == 9
    # refused on the host before anything is routed
    with pytest.raises(ValueError, match='beam groups'):
        dec.beam_search(fm, None, 4, 14, sampling=BeamSampling(0.7, 3), groups=BeamGroups(2, 0.5))
    with pytest.raises(ValueError, match='length penalty'):
        dec.beam_search(fm, None, 4, 14, sampling=BeamSampling(0.7, 3), length_penalty_weight=0.7)


# ---- the sampled-step reference itself -------------------------------------------------------------------------------------
END = 4


def test_ref_step_on_hand_made_inputs():
    """Two slots of one entry, V = 5.  Slot 0 is live, slot 1 finished.  With the noise given, slot 0 takes
    argmax(lp / T + g); the state adds the UNTEMPERED lp; the finished slot emits <EOS> whatever its noise."""
    lp = np.log(np.array([[[0.1, 0.4, 0.3, 0.15, 0.05], [0.2, 0.2, 0.2, 0.2, 0.2]]], np.float64))
    g = np.array([[[0.0, 0.0, 1.0, 0.0, 0.0], [9.0, 0.0, 0.0, 0.0, 0.0]]], np.float64)
    log_probs = np.array([[-1.0, -3.0]], np.float32)
    finished = np.array([[0, 1]], np.int32)
    lengths = np.array([[2, 2]], np.int64)
    r = sref.ref_select_sampled(lp, log_probs, finished, lengths, END, g, np.float32(1.0))
    np.testing.assert_array_equal(r['word'], [[2, END]])          # log .3 + 1 beats log .4
    np.testing.assert_array_equal(r['greedy'], [[1, END]])
    np.testing.assert_array_equal(r['parent'], [[0, 1]])
    np.testing.assert_allclose(r['log_probs'], [[-1.0 + np.log(0.3), -3.0]])
    np.testing.assert_array_equal(r['scores'], r['log_probs'])
    np.testing.assert_array_equal(r['finished'], [[0, 1]])
    np.testing.assert_array_equal(r['lengths'], [[3, 2]])
    # the margin is the live slot's: (log .3 + 1) - log .4 over GAP * max(1, |rank|)
    np.testing.assert_allclose(r['margin'], (np.log(0.3) + 1 - np.log(0.4)) / 1e-4)
    # a low temperature sharpens: log .3 / T + 1 < log .4 / T at T = 0.25
    r = sref.ref_select_sampled(lp, log_probs, finished, lengths, END, g, sref.inv_temp_of(0.25))
    np.testing.assert_array_equal(r['word'], [[1, END]])
    np.testing.assert_allclose(r['log_probs'], [[-1.0 + np.log(0.4), -3.0]])
    # a ban is -inf whatever the noise
    banned = lp.copy()
    banned[0, 0, 1] = -np.inf
    r = sref.ref_select_sampled(banned, log_probs, finished, lengths, END, g, sref.inv_temp_of(0.25))
    np.testing.assert_array_equal(r['word'], [[2, END]])
    # <EOS> ends the chain
    g2 = np.zeros_like(g)
    g2[0, 0, END] = 10.0
    r = sref.ref_select_sampled(lp, log_probs, finished, lengths, END, g2, np.float32(1.0))
    np.testing.assert_array_equal(r['word'], [[END, END]])
    np.testing.assert_array_equal(r['finished'], [[1, 1]])
    np.testing.assert_array_equal(r['lengths'], [[3, 2]])
