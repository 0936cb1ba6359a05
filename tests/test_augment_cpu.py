"""CPU side of `--cnn_input_augment_crop area` / `--cnn_input_augment_color fast|full`: the reference of the definition
(tests/augment_ref.py) against colorsys, the draw rule, the host loader path, the default stream, the command line and the
C boundary."""
import colorsys
import ctypes as C
import importlib.util
import os
import random
import re
import subprocess

import numpy as np
import pytest

from comic_amd import _lib as L, augment, inputs
from tests import augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
# The float32 formulation of tests/augment_ref.py against Python's colorsys in float64 on the inputs of
# test_colour_ops_against_colorsys: worst deviation measured 1.0016e-06 (the hue op; saturation 7.08e-07, h itself 9.7e-08,
# s 6.9e-08).  The bound is four times the worst.
MEASURED_WORST = 1.0016e-06
BOUND = 4 * MEASURED_WORST


def _pixels():
    """about 30k random 8-bit pixels and the edge pixels of the GPU colour test (black, white, greys, primaries, secondaries,
    clipping saturations, values brightness pushes out of range, hues that wrap), as [0,1] float32"""
    from tests.test_gpu_augment import _palette
    rng = np.random.default_rng(20261021)
    px = np.concatenate([rng.integers(0, 256, (30000, 3), dtype=np.uint8), _palette(8, 12).reshape(-1, 3)])
    return (px.astype(f32) * f32(1.0 / 255)).astype(f32), rng


def test_colour_ops_against_colorsys():
    """Saturation and hue of the reference (random factors per pixel) against colorsys in float64: within BOUND = 4 x the
    reference's own worst deviation (measured 1.0016e-06, so 4.0064e-06)."""
    c, rng = _pixels()
    n = len(c)
    fs = rng.uniform(0.5, 1.5, n).astype(f32)
    dh = rng.uniform(-0.2, 0.2, n).astype(f32)
    hsv = np.array([colorsys.rgb_to_hsv(*[float(v) for v in p]) for p in c])
    h, s, v = R.rgb_to_hsv(c)
    d = np.abs(h - hsv[:, 0])
    dev = dict(h=float(np.minimum(d, 1 - d).max()), s=float(np.abs(s - hsv[:, 1]).max()), v=float(np.abs(v - hsv[:, 2]).max()))
    want_sat = np.array([colorsys.hsv_to_rgb(a, min(max(b * float(f), 0.0), 1.0), m) for (a, b, m), f in zip(hsv, fs)])
    want_hue = np.array([colorsys.hsv_to_rgb((a + float(t)) % 1.0, b, m) for (a, b, m), t in zip(hsv, dh)])
    dev['saturation'] = float(np.abs(R.saturation(c, fs) - want_sat).max())
    dev['hue'] = float(np.abs(R.hue(c, dh) - want_hue).max())
    print('deviation from colorsys:', dev, 'bound', BOUND)
    assert dev['v'] == 0.0 and max(dev.values()) <= BOUND, dev
    assert h.min() >= 0.0 and h.max() < 1.0 and s.min() >= 0.0 and s.max() <= 1.0


def test_identities_of_the_reference():
    """Saturation factor 1 and hue 0 / +-1 within BOUND; brightness 0 exact; saturation 0 gives r = g = b = max.
    Contrast 1 is exact where the definition allows it: (v - m) * 1 + m in three float32 roundings returns v when v - m is
    exact, which Sterbenz's lemma gives for m / 2 <= v <= 2 m -- an image inside that range is checked bit for bit.  Outside it
    the difference rounds (by at most 2^-25 for |v - m| < 1) and so does the sum (at most 2^-25 for |v| <= 1): over all pixels
    the identity holds within 2^-24 = 5.96e-08, not exactly (measured on these pixels: 16 584 of 90 000 values move, by at most 1.49e-08)."""
    c, _ = _pixels()
    for got in (R.saturation(c, 1.0), R.hue(c, 0.0), R.hue(c, 1.0), R.hue(c, -1.0)):
        assert got.dtype == np.float32 and float(np.abs(got - c).max()) <= BOUND
    assert R.brightness(c, 0.0).tobytes() == c.tobytes()
    img = c[:30000].reshape(100, 300, 3)
    mid = (img * f32(0.25) + f32(0.375)).astype(f32)               # values in [0.375, 0.625], means about 0.5
    mean = R.channel_sums(mid) / (2.0 ** 32 * 30000)
    assert (mid >= mean / 2).all() and (mid <= 2 * mean).all()
    assert R.contrast(mid, 1.0).tobytes() == mid.tobytes()
    off = np.abs(R.contrast(img, 1.0) - img)
    print('contrast 1 on the whole range: worst %.3e, %d of %d values moved' % (off.max(), (off > 0).sum(), off.size))
    assert float(off.max()) <= 2.0 ** -24
    grey = R.saturation(c, 0.0)
    assert (grey == c.max(-1, keepdims=True)).all()
    # the mean is an integer sum: the same in any order of the pixels
    perm = np.random.default_rng(1).permutation(len(c))
    assert R.channel_sums(c).tolist() == R.channel_sums(c[perm]).tolist()
    assert abs(float(R.channel_sums(c)[0]) / (2.0 ** 32 * len(c)) - float(c[:, 0].astype(np.float64).mean())) < 1e-9


def test_product_colour_ops_equal_the_reference():
    c, _ = _pixels()
    img = c[:30000].reshape(100, 300, 3)
    for ops in R.ORDERINGS['full'] + R.ORDERINGS['fast'] + [[R.CONTRAST, 0, 0, 0], [0, 0, 0, 0]]:
        rec = R.record(ops=[o for o in ops if o], brightness=0.1, saturation=1.4, hue=-0.17, contrast=0.7)
        assert augment.distort_color(img, rec).tobytes() == R.distort(img, rec).tobytes(), ops


# ---- the draw rule ---------------------------------------------------------------------------------------------------------------
def _keys(n, seed=5):
    rng = random.Random(seed)
    return np.array([rng.getrandbits(64) for _ in range(n)], np.uint64)


def test_splitmix_is_the_librarys():
    src = open(os.path.join(os.path.dirname(L.__file__), 'csrc', 'splitmix.h')).read()
    for const in ('0x9E3779B97F4A7C15', '0xBF58476D1CE4E5B9', '0x94D049BB133111EB'):
        assert const in src
    keys = _keys(64)
    assert augment.splitmix64(keys).tolist() == [R.splitmix64(int(k)) for k in keys]
    assert R.splitmix64(0) == 0xE220A8397B1DCDAF                       # the published first output of splitmix64 seeded with 0
    assert augment.uniform(keys, 3).tolist() == [R.u01(int(k), 3) for k in keys]


def test_augment_params_equal_the_restated_rule():
    keys = _keys(300)
    rng = np.random.default_rng(2)
    hs, ws = rng.integers(1, 700, 300), rng.integers(1, 700, 300)
    for crop, color, amin, out in (('area', 'full', 0.35, (224, 224)), ('area', 'none', 0.05, (96, 128)),
                                   ('fixed', 'fast', 0.35, (224, 224)), ('area', 'fast', 1.0, (299, 299))):
        spec = augment.AugmentSpec(crop, color, amin, out[0], out[1], 256 if out[0] <= 256 else 342)
        ap = augment.augment_params(keys, hs, ws, spec)
        again = augment.augment_params(keys[::-1].copy(), hs[::-1], ws[::-1], spec)
        assert ap.aug.tobytes() == again.aug[::-1].tobytes()                        # per key, whatever its neighbours
        assert ap.aug.dtype.itemsize == 48
        for i in range(len(keys)):
            rec, flip, oy, ox = R.expected_params(int(keys[i]), int(hs[i]), int(ws[i]), crop, color, amin, out[0], out[1],
                                                  spec.resize)
            assert ap.aug[i].tobytes() == rec.tobytes(), (crop, color, i, ap.aug[i], rec)
            assert (bool(ap.flip[i]), int(ap.oy[i]), int(ap.ox[i])) == (flip, oy, ox)
        assert ap.contrast == (color == 'full')


def test_boxes_lie_inside_and_in_range():
    """w = round(sqrt(area * aspect)) and h = round(sqrt(area / aspect)) move each side by at most 1/2 from the real-valued box:
    the true area lies in [(w - 1/2)(h - 1/2), (w + 1/2)(h + 1/2)] and the true aspect in [(w - 1/2) / (h + 1/2),
    (w + 1/2) / (h - 1/2)], and these intervals must meet [area_min H W, H W] and [3/4, 4/3]."""
    keys = _keys(1000, 9)
    rng = np.random.default_rng(3)
    for amin in (0.35, 0.05):
        H, W = rng.integers(8, 700, 1000), rng.integers(8, 700, 1000)
        cy, cx, ch, cw, fb = augment.draw_boxes(keys, H, W, amin)
        assert (cy >= 0).all() and (cx >= 0).all() and (ch >= 1).all() and (cw >= 1).all()
        assert (cy + ch <= H).all() and (cx + cw <= W).all()
        ok = ~fb
        assert ok.sum() > 500 and fb.any()                  # (sides of 8 ... 700: the most oblong images take the fallback)
        assert not augment.draw_boxes(keys, np.full(1000, 480), np.full(1000, 640), amin)[4].any()
        assert ((cw + 0.5) * (ch + 0.5) >= amin * H * W)[ok].all() and ((cw - 0.5) * (ch - 0.5) <= H * W)[ok].all()
        assert ((cw + 0.5) / (ch - 0.5) >= 3 / 4)[ok].all() and ((cw - 0.5) / (ch + 0.5) <= 4 / 3)[ok].all()
        assert len(set(cy[ok].tolist())) > 50 and len(set(cx[ok].tolist())) > 50          # the origin moves
    # a 1 x N and an N x 1 source: no attempt fits, the centred largest box of an aspect in the range
    n = 64
    for H, W, want in ((1, n, (0, (n - 1) // 2, 1, 1)), (n, 1, ((n - 1) // 2, 0, 1, 1))):
        cy, cx, ch, cw, fb = augment.draw_boxes(keys, np.full(1000, H), np.full(1000, W), 0.35)
        assert fb.all() and {(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(cy, cx, ch, cw)} == {want}
    cy, cx, ch, cw, fb = augment.draw_boxes(keys[:4], np.full(4, 100), np.full(4, 30), 1.0)      # too narrow for the whole area
    assert fb.all() and (ch == 40).all() and (cw == 30).all() and (cy == 30).all() and (cx == 0).all()


def test_orderings_cover_all_values():
    keys = _keys(1000, 4)
    for color, count in (('full', 4), ('fast', 2)):
        ap = augment.augment_params(keys, np.full(1000, 64), np.full(1000, 64), augment.AugmentSpec('fixed', color))
        seen = {tuple(o) for o in ap.aug['ops'].tolist()}
        assert seen == {tuple(o) for o in R.ORDERINGS[color]} and len(seen) == count
        assert abs(float(ap.flip.mean()) - 0.5) < 0.06
        assert np.abs(ap.aug['brightness']).max() <= 32 / 255 and 0.5 <= ap.aug['saturation'].min() <= ap.aug['saturation'].max() <= 1.5
        if color == 'full':
            assert np.abs(ap.aug['hue']).max() <= 0.2 and 0.5 <= ap.aug['contrast'].min() <= ap.aug['contrast'].max() <= 1.5
        assert (ap.aug['mode'] == L.AUG_LEGACY).all() and ap.oy.min() >= 0 and ap.oy.max() <= 32 and len(set(ap.oy.tolist())) == 33


# ---- the host loader path --------------------------------------------------------------------------------------------------------
def test_host_path_equals_the_reference():
    rng = np.random.default_rng(8)
    keys = _keys(12, 2)
    for crop, color in (('area', 'full'), ('fixed', 'fast'), ('area', 'none'), ('fixed', 'full')):
        for (h, w), out in (((37, 53), (16, 24)), ((300, 201), (64, 48))):
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            ap = augment.augment_params(keys, [h] * 12, [w] * 12, augment.AugmentSpec(crop, color, 0.35, out[0], out[1]))
            for i in range(12):
                got = inputs.preprocess_image(img, out[0], out[1], True, None, (bool(ap.flip[i]), int(ap.oy[i]), int(ap.ox[i])),
                                              ap.aug[i])
                want = R.preprocess(img, out[0], out[1], bool(ap.flip[i]), ap.aug[i], int(ap.oy[i]), int(ap.ox[i]))
                assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (crop, color, h, w, i)
    # without a record: the function of before
    img = rng.integers(0, 256, (50, 70, 3), dtype=np.uint8)
    plain = inputs.preprocess_image(img, 224, 224, True, None, (True, 3, 9))
    assert plain.tobytes() == R.preprocess(img, 224, 224, True, R.record(R.LEGACY), 3, 9).tobytes()


# ---- defaults: nothing changes -----------------------------------------------------------------------------------------------------
def _train_module():
    spec = importlib.util.spec_from_file_location('cli_train_augment', os.path.join(ROOT, 'src', 'train.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_default_stream_is_unchanged(tmp_path):
    """draw_augmentation consumes what it consumed: a coin and two window origins per image, from random.Random."""
    a, b = random.Random(48964896), random.Random(48964896)
    for _ in range(200):
        want = (b.random() < 0.5, b.randrange(0, 256 - 224 + 1), b.randrange(0, 256 - 224 + 1))
        assert inputs.draw_augmentation(True, 224, 224, a) == want
    assert inputs.draw_augmentation(False, 224, 224, a) == (False, 16, 16) and a.random() == b.random()
    # a manager with the flags at their defaults draws through it and keeps no spec; its batches are preprocess_image's
    from tests import tiny_dataset
    from comic_amd import configuration as conf
    ds = tiny_dataset.make(str(tmp_path / 'mscoco'), n_train=8, n_valid=2, n_test=2)
    kw = dict(dataset_dir=ds, dataset_file_pattern='mscoco_{}_w5_s20_include_restval', cnn_name='inception_v1',
              cnn_input_size=[224, 224], cnn_input_augment=True, batch_size_train=2, batch_size_eval=2, max_epoch=1, rand_seed=3,
              token_type='radix', radix_base=256, loader_threads=2, loader_prefetch=1)
    m = inputs.InputManager_Radix(conf.Config(**kw))
    try:
        assert m._aug_spec is None
        ims, _ = next(m.batch_train)
        assert ims.shape == (2, 224, 224, 3)
    finally:
        m.close()


def test_defaults_add_no_key_and_keep_the_directory(tmp_path):
    train = _train_module()
    kw, _, _ = train.build_kwargs(train.create_parser().parse_args(['--log_root', str(tmp_path)]))
    assert not [k for k in kw if k.startswith('cnn_input_augment_')] and kw['cnn_input_augment'] is True
    assert os.path.basename(kw['log_path']) == 'radix_b256_add_LN_softmax_h8_tie_lstm_run_01'
    for argv, suffix, keys in ((['--cnn_input_augment_crop', 'area'], '_augA0.35', dict(cnn_input_augment_crop='area',
                                                                                      cnn_input_augment_area_min=0.35)),
                               (['--cnn_input_augment_color', 'full'], '_augCfull', dict(cnn_input_augment_color='full')),
                               (['--cnn_input_augment_color', 'fast'], '_augCfast', dict(cnn_input_augment_color='fast')),
                               (['--cnn_input_augment_crop', 'area', '--cnn_input_augment_area_min', '0.5',
                                 '--cnn_input_augment_color', 'full'], '_augA0.5Cfull',
                                dict(cnn_input_augment_crop='area', cnn_input_augment_area_min=0.5, cnn_input_augment_color='full'))):
        kw, _, _ = train.build_kwargs(train.create_parser().parse_args(['--log_root', str(tmp_path)] + argv))
        assert os.path.basename(kw['log_path']) == 'radix_b256_add_LN_softmax_h8_tie_lstm%s_run_01' % suffix
        assert {k: v for k, v in kw.items() if k.startswith('cnn_input_augment_')} == keys
    # the suffix sits beside the other stages' ones
    kw, _, _ = train.build_kwargs(train.create_parser().parse_args(
        ['--log_root', str(tmp_path), '--cnn_input_augment_color', 'fast', '--label_smoothing', '0.1']))
    assert os.path.basename(kw['log_path']) == 'radix_b256_add_LN_softmax_h8_tie_lstm_augCfast_ls0.1_run_01'
    from types import SimpleNamespace as NS
    assert augment.spec_from_config(NS(cnn_input_size=[224, 224])) is None
    s = augment.spec_from_config(NS(cnn_input_size=[224, 200], cnn_input_augment_color='fast'))
    assert (s.crop, s.color, s.area_min, s.out_h, s.out_w) == ('fixed', 'fast', 0.35, 224, 200)


def test_cli_refusals_before_the_gpu(tmp_path):
    train = _train_module()
    never = ['--log_root', '/nonexistent/never/created']
    for argv, word in ((['--cnn_input_augment', '', '--cnn_input_augment_crop', 'area'], 'need --cnn_input_augment True'),
                       (['--cnn_input_augment', '', '--cnn_input_augment_color', 'fast'], 'need --cnn_input_augment True'),
                       (['--cnn_input_augment', '', '--cnn_input_augment_area_min', '0.5'], 'need --cnn_input_augment True'),
                       (['--cnn_input_augment_crop', 'area', '--cnn_input_augment_area_min', '0'], r'\(0, 1\]'),
                       (['--cnn_input_augment_crop', 'area', '--cnn_input_augment_area_min', '1.5'], r'\(0, 1\]'),
                       (['--cnn_input_augment_crop', 'area', '--cnn_input_augment_area_min', 'nan'], r'\(0, 1\]'),
                       (['--cnn_input_augment_area_min', '0.5'], 'needs --cnn_input_augment_crop area')):
        with pytest.raises(ValueError, match=word):
            train.main(argv + never)
    assert not os.path.exists('/nonexistent/never/created')
    for argv in (['--cnn_input_augment_crop', 'box'], ['--cnn_input_augment_color', 'all']):
        with pytest.raises(SystemExit):
            train.create_parser().parse_args(argv)
    train.refuse_bad_augment_options(vars(train.create_parser().parse_args(['--cnn_input_augment', ''])))
    train.refuse_bad_augment_options(vars(train.create_parser().parse_args(
        ['--train_mode', 'scst', '--cnn_input_augment_crop', 'area', '--cnn_input_augment_area_min', '1', '--cnn_input_augment_color',
         'full'])))


# ---- the C boundary ----------------------------------------------------------------------------------------------------------------
def test_record_layout_and_entries():
    """include/comic_hip.h, _lib and the cross-compiled library agree on comic_image_aug and on the three entries, argument by
    argument; each entry is its plain form with `aug, contrast, aug_ws` behind `desc`."""
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    fields = re.search(r'typedef struct comic_image_aug \{(.*?)\}', header, flags=re.S).group(1)
    names = [re.sub(r'\[\d+\]', '', v).strip() for f in fields.split(';') if f.strip()
             for v in f.strip().split(None, 1)[1].split(',')]
    assert names == [n for n, _ in L.ImageAug._fields_] == list(np.dtype(L.IMAGE_AUG_DTYPE).names) == list(R.AUG_DTYPE.names)
    assert C.sizeof(L.ImageAug) == np.dtype(L.IMAGE_AUG_DTYPE).itemsize == R.AUG_DTYPE.itemsize == 48
    for n in names:
        assert getattr(L.ImageAug, n).offset == np.dtype(L.IMAGE_AUG_DTYPE).fields[n][1] == R.AUG_DTYPE.fields[n][1], n
    dev = open(os.path.join(os.path.dirname(L.__file__), 'csrc', 'augment_dev.h')).read()
    assert 'static_assert(sizeof(ImgAug) == sizeof(comic_image_aug) && sizeof(ImgAug) == 48' in dev
    assert C.sizeof(L.ImageDesc) == 40 and 'static_assert(sizeof(ImgDesc) == 40' in dev
    for const, val in (('COMIC_AUG_LEGACY', L.AUG_LEGACY), ('COMIC_AUG_BOX', L.AUG_BOX), ('COMIC_AUG_OP_NONE', L.AUG_OP_NONE),
                       ('COMIC_AUG_OP_BRIGHTNESS', L.AUG_OP_BRIGHTNESS), ('COMIC_AUG_OP_SATURATION', L.AUG_OP_SATURATION),
                       ('COMIC_AUG_OP_HUE', L.AUG_OP_HUE), ('COMIC_AUG_OP_CONTRAST', L.AUG_OP_CONTRAST)):
        assert int(re.search(r'\b%s = (\d+)' % const, header).group(1)) == val
    assert (R.LEGACY, R.BOX, R.NONE, R.BRIGHTNESS, R.SATURATION, R.HUE, R.CONTRAST) == (
        L.AUG_LEGACY, L.AUG_BOX, L.AUG_OP_NONE, L.AUG_OP_BRIGHTNESS, L.AUG_OP_SATURATION, L.AUG_OP_HUE, L.AUG_OP_CONTRAST)
    assert augment.ORDERINGS['full'] == tuple(tuple(o) for o in R.ORDERINGS['full'])
    assert augment.ORDERINGS['fast'] == tuple(tuple(o) for o in R.ORDERINGS['fast'])
    decls = {name: [a.strip() for a in args.split(',')]
             for name, args in re.findall(r'\bint\s+(comic_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', header)}

    def ctype(a):
        if '*' in a:
            return L.P
        return {'int': C.c_int, 'float': C.c_float, 'int64_t': C.c_int64}[a.replace('const', '').split()[0]]
    pairs = (('comic_image_preprocess_aug', 'comic_image_preprocess'), ('comic_jpeg_preprocess_aug', 'comic_jpeg_preprocess'),
             ('comic_jpeg_preprocess_packed_aug', 'comic_jpeg_preprocess_packed'))
    extra = ['const void* aug', 'int contrast', 'void* aug_ws']
    for name, plain in pairs:
        res, args = L._SIGS[name]
        assert res is C.c_int and [ctype(a) for a in decls[name]] == list(args), name
        at = decls[plain].index('const void* desc') + 1
        assert decls[name] == decls[plain][:at] + extra + decls[plain][at:], name
        assert name in L.EXPORTED_SYMBOLS
    defined = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in defined.splitlines() if line.strip())
    assert {p[0] for p in pairs} <= exported
    src = open(os.path.join(os.path.dirname(L.__file__), 'csrc', 'Makefile')).read()
    assert 'augment_dev.h' in src
    for f in ('preprocess.hip', 'jpeg_pixels.hip'):              # one copy of the records and the lerp, in the shared header
        text = open(os.path.join(os.path.dirname(L.__file__), 'csrc', f)).read()
        assert '#include "augment_dev.h"' in text and 'struct ImgDesc' not in text and 'float lerp_rn' not in text
