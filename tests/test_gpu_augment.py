"""Training augmentation inside the device preprocessing launches (comic_image_preprocess_aug, comic_jpeg_preprocess_aug,
comic_jpeg_preprocess_packed_aug; csrc/augment_dev.h): the box geometry, the colour ops, the two-pass contrast mean, the
legacy geometry and the loader paths.  Every comparison is bit for bit against tests/augment_ref.py; outputs start as NaN."""
import os

import numpy as np
import pytest

from comic_amd import _lib as L
from tests import augment_ref as R

pytestmark = pytest.mark.gpu

B, S, H, C = R.BRIGHTNESS, R.SATURATION, R.HUE, R.CONTRAST


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def _desc(images, flips, windows=None, resize=256):
    from comic_amd import inputs
    n = len(images)
    desc = np.zeros(n, inputs.DevicePreprocessor._DESC_DTYPE)
    sizes = np.array([im.size for im in images], np.int64)
    off = np.concatenate([[0], np.cumsum((sizes + 15) // 16 * 16)])
    desc['offset'] = off[:-1]
    desc['in_h'], desc['in_w'] = [im.shape[0] for im in images], [im.shape[1] for im in images]
    desc['flip'] = flips
    if windows is not None:
        desc['oy'], desc['ox'] = [w[0] for w in windows], [w[1] for w in windows]
    desc['sy'] = (desc['in_h'] / resize).astype(np.float32)
    desc['sx'] = (desc['in_w'] / resize).astype(np.float32)
    blob = np.zeros(int(off[-1]) + 64, np.uint8)
    for o, im in zip(off, images):
        blob[o:o + im.size] = im.reshape(-1)
    return desc, blob


def _run_blob(images, flips, recs, out_h, out_w, windows=None, ws=None, contrast=None, resize=256):
    """comic_image_preprocess_aug of one batch -> [n, out_h, out_w, 3] float32 (numpy)."""
    import torch
    n = len(images)
    desc, blob = _desc(images, flips, windows, resize)
    aug = np.array(recs, R.AUG_DTYPE)
    assert aug.dtype.itemsize == 48
    if contrast is None:
        contrast = int((aug['ops'] == C).any())
    out = torch.full((n, out_h, out_w, 3), float('nan'), dtype=torch.float32, device='cuda')
    if ws is None:
        ws = torch.full((3 * n,), -12345, dtype=torch.int64, device='cuda')          # stale words: the entry clears them
    db, dd, da = _dev(blob), _dev(desc), _dev(aug)
    L.check(L.load().comic_image_preprocess_aug(db.data_ptr(), dd.data_ptr(), da.data_ptr(), contrast, ws.data_ptr(), n,
                                                out.data_ptr(), out_h, out_w, resize, L.stream_ptr()), 'image_preprocess_aug')
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _want(images, flips, recs, out_h, out_w, windows=None):
    windows = windows or [(0, 0)] * len(images)
    return np.stack([R.preprocess(im, out_h, out_w, bool(f), r, w[0], w[1]) for im, f, r, w in zip(images, flips, recs, windows)])


def _same(got, want, names=None):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert not np.isnan(got).any(), 'an output element was not written'
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if len(bad):
        at = tuple(int(v) for v in bad[0])
        raise AssertionError('%d elements differ; first at %s%s: got %r, want %r' % (
            len(bad), at, ' (%s)' % (names[at[0]],) if names else '', got[at], want[at]))


# ---- 1. geometry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('out_hw', [(8, 12), (16, 24)])
def test_box_geometry_equals_the_reference(out_hw):
    """RGB-blob entry, no ops.  Boxes per source: the whole image, 1 x 1 at the last pixel (every output equals it), a box
    touching the bottom-right corner, 3 x 4 (up-scaled at 16 x 24) where it fits -- the whole 37 x 53 image is the down-scale
    to 8 x 12.  Each with and without the flip, all in one launch."""
    out_h, out_w = out_hw
    rng = np.random.default_rng(3)
    images, flips, recs, names = [], [], [], []
    for (h, w) in ((5, 7), (1, 9), (9, 1), (37, 53)):
        src = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        boxes = [(0, 0, h, w), (h - 1, w - 1, 1, 1), (h - (h + 1) // 2, w - (w + 1) // 2, (h + 1) // 2, (w + 1) // 2)]
        if h >= 4 and w >= 6:
            boxes.append((1, 2, 3, 4))
        for box in boxes:
            for flip in (0, 1):
                images.append(src)
                flips.append(flip)
                recs.append(R.record(R.BOX, box, out_hw))
                names.append('%dx%d box %s flip %d' % (h, w, box, flip))
    got = _run_blob(images, flips, recs, out_h, out_w)
    _same(got, _want(images, flips, recs, out_h, out_w), names)
    for i, name in enumerate(names):
        if recs[i]['ch'] == 1 and recs[i]['cw'] == 1:
            px = images[i][-1, -1].astype(np.float32) * np.float32(1.0 / 255)
            assert (got[i] == (px - np.float32(0.5)) * np.float32(2)).all(), name


# ---- 2. colour ---------------------------------------------------------------------------------------------------------------------
def _palette(out_h, out_w):
    """out_h x out_w pixels read through a box of the output's size (the taps are the pixels themselves): black, white, greys
    (d = 0), the primaries and secondaries (ties between maxima), saturations that clip at 1 under f = 1.5, values that
    brightness +-32/255 pushes outside [0, 1], hues next to 0 on both sides (they wrap under +-0.2), the rest random."""
    fixed = [(0, 0, 0), (255, 255, 255), (1, 1, 1), (128, 128, 128), (254, 254, 254), (37, 37, 37),
             (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255),
             (200, 200, 0), (90, 0, 90), (0, 17, 17), (255, 255, 254), (255, 254, 255), (254, 255, 255),
             (255, 40, 60), (10, 200, 30), (3, 2, 250), (240, 10, 10), (100, 20, 20),
             (250, 250, 3), (2, 7, 1), (255, 128, 0), (0, 3, 12), (251, 255, 249), (16, 16, 15),
             (200, 21, 20), (200, 20, 21), (255, 1, 0), (255, 0, 1), (90, 10, 11), (180, 50, 47), (30, 200, 200), (200, 30, 200),
             (60, 60, 200), (61, 60, 200), (60, 61, 200)]
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (out_h * out_w, 3), dtype=np.uint8)
    img[:len(fixed)] = fixed
    return img.reshape(out_h, out_w, 3)


def test_colour_ops_equal_the_reference():
    """Each op alone at both ends of its range, the four `full` orderings and the two `fast` ones, as one batch."""
    out_hw = (8, 12)
    img = _palette(*out_hw)
    par = dict(brightness=-0.0731, saturation=1.37, hue=0.1234, contrast=0.61)
    lists = [('brightness +', [B], dict(brightness=32.0 / 255)), ('brightness -', [B], dict(brightness=-32.0 / 255)),
             ('saturation 1.5', [S], dict(saturation=1.5)), ('saturation 0.5', [S], dict(saturation=0.5)),
             ('hue +0.2', [H], dict(hue=0.2)), ('hue -0.2', [H], dict(hue=-0.2)),
             ('contrast 1.5', [C], dict(contrast=1.5)), ('contrast 0.5', [C], dict(contrast=0.5))]
    lists += [('full %d' % k, o, par) for k, o in enumerate(R.ORDERINGS['full'])]
    lists += [('fast %d' % k, o, par) for k, o in enumerate(R.ORDERINGS['fast'])]
    recs = [R.record(R.BOX, (0, 0) + out_hw, out_hw, [o for o in ops if o], **kw) for _, ops, kw in lists]
    images, flips = [img] * len(recs), [0] * len(recs)
    got = _run_blob(images, flips, recs, *out_hw)
    _same(got, _want(images, flips, recs, *out_hw), [l[0] for l in lists])
    assert got.min() >= -1.0 and got.max() <= 1.0                              # distort_color's final clamp


# ---- 3. the contrast sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('out_hw', [(13, 19), (24, 31)])
def test_contrast_sums_are_exact_repeatable_and_cleared(out_hw):
    """247 pixels are less than one workgroup, 744 are three with a tail.  A batch of four op lists (one without contrast, one
    with no op at all); the same call twice gives the same bytes; a second batch through the SAME workspace is right too."""
    import torch
    out_h, out_w = out_hw

    def batch(seed):
        r = np.random.default_rng(seed)
        images = [r.integers(0, 256, (41, 57, 3), dtype=np.uint8), r.integers(0, 256, (29, 33, 3), dtype=np.uint8),
                  r.integers(0, 256, (out_h, out_w, 3), dtype=np.uint8), r.integers(100, 256, (50, 64, 3), dtype=np.uint8)]
        recs = [R.record(R.BOX, (3, 5, 30, 41), out_hw, [B, S, H, C], brightness=0.11, saturation=0.7, hue=-0.15, contrast=1.45),
                R.record(R.BOX, (0, 0, 29, 33), out_hw, [S, B], brightness=-0.1, saturation=1.3),
                R.record(R.BOX, (0, 0, out_h, out_w), out_hw, []),
                R.record(R.BOX, (7, 9, 40, 50), out_hw, [C, H, B, S], brightness=0.12, saturation=1.2, hue=0.05, contrast=0.55)]
        return images, [1, 0, 0, 1], recs
    images, flips, recs = batch(1)
    ws = torch.full((12,), 7, dtype=torch.int64, device='cuda')
    first = _run_blob(images, flips, recs, out_h, out_w, ws=ws)
    sums = ws.cpu().numpy().reshape(4, 3)
    second = _run_blob(images, flips, recs, out_h, out_w, ws=ws)
    _same(first, _want(images, flips, recs, out_h, out_w))
    assert first.tobytes() == second.tobytes()
    # the words of the workspace are the reference's integer sums in front of the contrast op; images without one stay 0
    c0 = R.hue(R.saturation(R.brightness(R.geometry(images[0], out_h, out_w, True, recs[0]), 0.11), 0.7), -0.15)
    c3 = R.geometry(images[3], out_h, out_w, True, recs[3])
    assert sums[0].tolist() == R.channel_sums(c0).tolist() and sums[3].tolist() == R.channel_sums(c3).tolist()
    assert not sums[1].any() and not sums[2].any()
    images, flips, recs = batch(2)
    images, flips, recs = images[::-1], flips[::-1], recs[::-1]     # other lists on the same slots of the workspace
    _same(_run_blob(images, flips, recs, out_h, out_w, ws=ws), _want(images, flips, recs, out_h, out_w))


# ---- 4. the JPEG entries -----------------------------------------------------------------------------------------------------------
def test_jpeg_entries_equal_the_blob_entry_and_the_reference(golden_dir, tmp_path):
    """The committed JPEG set (4:2:0, 4:2:2, 4:4:4, restart markers, optimised tables, grey) through the dense and the packed
    entry, one image of the batch on the PIL path (ncomp == 0, its pixels in the RGB blob): equal to the RGB-blob entry on PIL's
    pixels of the same files and to the reference."""
    import torch
    from tests.test_gpu_jpeg import _submit_packed
    from tests.test_jpeg_split import _split
    g = np.load(os.path.join(golden_dir, 'jpeg_split_golden.npz'))
    names = sorted(k[:-4] for k in g.files if k.endswith('.jpg'))
    assert len(names) == 6 and 'grey_q80' in names
    paths, rgb = [], []
    for nm in names:
        p = str(tmp_path / (nm + '.jpg'))
        with open(p, 'wb') as f:
            f.write(g[nm + '.jpg'].tobytes())
        paths.append(p)
        rgb.append(g[nm + '.rgb'])
    n, out_hw = len(names), (16, 24)
    infos, status, packed, total = _submit_packed(paths)
    assert (status == 0).all()
    dense = np.zeros(total, np.int16)
    for i, nm in enumerate(names):
        rc, _, coef = _split(g[nm + '.jpg'].tobytes())
        assert rc == 0
        dense[int(infos['coef_base'][i]):int(infos['coef_base'][i]) + coef.size] = coef
    pil = 2
    max_blocks = int(infos['coef_count'].max()) // 64
    infos = infos.copy()
    infos['ncomp'][pil] = 0
    full = R.ORDERINGS['full']
    recs, flips, windows = [], [], []
    for i, im in enumerate(rgb):
        h, w = im.shape[:2]
        box = [(0, 0, h, w), (h // 3, w // 4, h // 2, w // 2), (h - 9, w - 13, 9, 13)][i % 3]
        recs.append(R.record(R.BOX if i != 4 else R.LEGACY, box, out_hw, full[i % 4], brightness=0.02 * i - 0.05,
                             saturation=0.6 + 0.15 * i, hue=0.07 * i - 0.2, contrast=0.5 + 0.19 * i))
        flips.append(i % 2)
        windows.append((5 * i, 7 * i))
    want = _want(rgb, flips, recs, *out_hw, windows=windows)
    _same(_run_blob(rgb, flips, recs, *out_hw, windows=windows), want, names)
    desc, blob = _desc(rgb, flips, windows)                      # (offsets into a blob of all the images: only `pil`'s is read)
    aug = np.array(recs, R.AUG_DTYPE)
    lib = L.load()
    for entry, coef in (('comic_jpeg_preprocess_aug', torch.from_numpy(dense).cuda()),
                        ('comic_jpeg_preprocess_packed_aug', torch.from_numpy(packed.view(np.int16)).cuda())):
        out = torch.full((n,) + out_hw + (3,), float('nan'), dtype=torch.float32, device='cuda')
        planes = torch.zeros(total + 4096, dtype=torch.uint8, device='cuda')
        ws = torch.full((3 * n,), -1, dtype=torch.int64, device='cuda')
        di, dd, da, db = _dev(infos), _dev(desc), _dev(aug), _dev(blob)
        L.check(getattr(lib, entry)(coef.data_ptr(), di.data_ptr(), n, max_blocks, planes.data_ptr(), db.data_ptr(), dd.data_ptr(),
                                    da.data_ptr(), 1, ws.data_ptr(), out.data_ptr(), out_hw[0], out_hw[1], 256, L.stream_ptr()),
                entry)
        torch.cuda.synchronize()
        _same(out.cpu().numpy(), want, ['%s %s' % (entry, nm) for nm in names])


# ---- 5. the legacy geometry --------------------------------------------------------------------------------------------------------
def test_legacy_geometry_reproduces_the_plain_entry_and_takes_colour_ops():
    import torch
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((60, 80), (300, 257), (9, 200), (256, 256))]
    flips, windows = [0, 1, 1, 0], [(0, 0), (32, 32), (7, 19), (32, 0)]
    n, out = len(images), 224
    plain = [R.record(R.LEGACY) for _ in images]
    desc, blob = _desc(images, flips, windows)
    ref = torch.full((n, out, out, 3), float('nan'), dtype=torch.float32, device='cuda')
    db, dd = _dev(blob), _dev(desc)
    L.check(L.load().comic_image_preprocess(db.data_ptr(), dd.data_ptr(), n, ref.data_ptr(), out, out, 256, L.stream_ptr()), 'pre')
    torch.cuda.synchronize()
    got = _run_blob(images, flips, plain, out, out, windows)
    _same(got, ref.cpu().numpy())
    fast = [R.record(R.LEGACY, ops=R.ORDERINGS['fast'][i % 2], brightness=0.1 - 0.06 * i, saturation=0.55 + 0.3 * i)
            for i in range(n)]
    _same(_run_blob(images, flips, fast, out, out, windows), _want(images, flips, fast, out, out, windows))


# ---- 6. the loader -----------------------------------------------------------------------------------------------------------------
def test_loader_paths_give_identical_augmented_batches(tmp_path):
    """InputManager with `area` + `full` on the tiny dataset: the split-JPEG, DecodePool, in-thread and host paths yield the same
    batches for a seed, a second run repeats them, and two data-parallel ranks draw different augmentations."""
    import torch
    from tests import tiny_dataset
    from comic_amd import inputs, configuration as conf
    ds = tiny_dataset.make(str(tmp_path / 'mscoco'), n_train=24, n_valid=4, n_test=4)
    kw = dict(dataset_dir=ds, dataset_file_pattern='mscoco_{}_w5_s20_include_restval', cnn_name='inception_v3',
              cnn_input_size=[96, 128], cnn_input_augment=True, batch_size_train=4, batch_size_eval=2, max_epoch=3,
              rand_seed=7, token_type='radix', radix_base=256, loader_threads=4, loader_prefetch=2,
              cnn_input_augment_crop='area', cnn_input_augment_color='full')
    variants = dict(split=dict(loader_split_jpeg=True), pool=dict(loader_split_jpeg=False, loader_processes=2),
                    thread=dict(loader_split_jpeg=False), host=dict(loader_split_jpeg=False), again=dict(loader_split_jpeg=True))
    managers = {k: inputs.InputManager_Radix(conf.Config(**dict(kw, **v))) for k, v in variants.items()}
    ranks = [inputs.InputManager_Radix(conf.Config(dp_world=2, dp_rank=r, loader_split_jpeg=False, **kw)) for r in (0, 1)]
    try:
        for k, m in managers.items():
            if k != 'host':
                m.enable_device_preprocess('cuda:0')
        assert managers['split']._jpeg_pool is not None and managers['pool']._decode_pool is not None
        on_device = {k: 0 for k in managers}
        for step in range(6):
            batches = {k: next(m.batch_train) for k, m in managers.items()}
            want_im, want_cap = torch.as_tensor(batches['host'][0]).cpu(), batches['host'][1]
            assert tuple(want_im.shape) == (4, 96, 128, 3) and not torch.isnan(want_im).any()
            for k, (im, cap) in batches.items():
                on_device[k] += int(torch.is_tensor(im) and im.is_cuda)
                assert torch.equal(torch.as_tensor(im).cpu(), want_im), (k, step)
                np.testing.assert_array_equal(cap, want_cap)
        assert on_device['host'] == 0 and min(v for k, v in on_device.items() if k != 'host') >= 2, on_device
        a, b = next(ranks[0].batch_train)[0], next(ranks[1].batch_train)[0]
        assert not np.array_equal(a, b)
        # evaluation never augments: the plain central crop
        ev = next(managers['host'].batch_eval)[0]
        plain = inputs.InputManager_Radix(conf.Config(**{k: v for k, v in kw.items() if not k.startswith('cnn_input_augment_')},
                                                      loader_split_jpeg=False))
        ranks.append(plain)
        assert np.array_equal(ev, next(plain.batch_eval)[0])
    finally:
        for m in list(managers.values()) + ranks:
            m.close()
