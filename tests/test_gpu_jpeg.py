"""Device half of the split JPEG decoder (csrc/jpeg_pixels.hip) bit for bit at libjpeg's edge cases: comic_jpeg_pixels, and the
two kernels behind the loader's entry point comic_jpeg_preprocess_packed (the packed inverse DCT and the fused taps), over
samplings x sizes x qualities, saturating content whose AC coefficients need the two-word entries of the packed form, one-row and
one-column strips, images of one block per component, and batches that carry PIL-path images (ncomp == 0).

Every comparison is exact.  The references do not come from the code under test: PIL's decode of the same bytes (`_pil`),
oracle/jpeg_ref.py (pinned to PIL by the CPU tests of tests/test_jpeg_split.py) for the component planes, and
oracle/preprocess_ref.py on PIL's pixels for the network input.  Each test is one batch and one launch per entry point."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from comic_amd import _lib as L
from oracle import jpeg_ref, preprocess_ref
from tests.test_jpeg_split import _encode, _photo, _pil, _split

pytestmark = pytest.mark.gpu

SIZES = ((160, 120), (159, 107), (83, 125), (17, 9), (8, 8), (9, 33), (100, 1), (5, 200), (161, 3),     # the CPU matrix
         (256, 256), (255, 257),                   # identity scale of the 256 resize / one pixel either side of it
         (515, 16), (259, 10))                     # more than one 64-thread group per row of jpeg_colour_kernel, width % 4 != 0
QUALITIES = (35, 85, 98)
CORNERS = ((0, 0), (0, 32), (32, 0), (32, 32))     # (oy, ox) of a 224 window in the 256 x 256 resize
GUARD = 4096
_SAMPLING = {(1, 1): 0, (2, 1): 1, (2, 2): 2}


class _Image(object):
    __slots__ = ('name', 'data', 'info', 'coef', 'rgb')

    def __init__(self, name, data, info, coef):
        self.name, self.data, self.coef = name, data, coef
        self.info = np.frombuffer(bytes(info), L.JPEG_INFO_DTYPE).copy()       # one record
        self.rgb = _pil(data)

    @property
    def sampling(self):
        return _SAMPLING[(int(self.info['hmax'][0]), int(self.info['vmax'][0]))]

    def plane_coef(self, c):
        i = self.info[0]
        off = int(i['coef_off'][c])
        return self.coef[off:off + int(i['blocks_w'][c]) * int(i['blocks_h'][c]) * 64].reshape(-1, 64)


def _two_word(ac):
    return int(np.count_nonzero((ac < -512) | (ac > 511)))


@functools.lru_cache(maxsize=None)
def _inputs():
    """-> (images, counts): the shared set, and what it holds of the things it is there for.  Asserts its own conditions: a set
    that lost its two-word entries or its full blocks must fail every test, not pass them quietly."""
    images = []

    def add(name, arr, **kw):
        data = _encode(arr, **kw)
        rc, info, coef = _split(data)
        if rc == L.JPEG_UNSUPPORTED:
            return False
        assert rc == 0, (name, rc)
        images.append(_Image(name, data, info, coef))
        return True
    matrix = 0
    for sub in (0, 1, 2):
        for (w, h) in SIZES:
            img = _photo(h, w, seed=w + h)
            for q in QUALITIES:
                if add('photo_%dx%d_q%d_s%d' % (w, h, q, sub), img, quality=q, subsampling=sub):
                    matrix += 1
                else:
                    assert sub and (w + 1) // 2 <= 2, (w, h, q, sub)          # libjpeg's box filter: left to PIL
    assert matrix >= 90, matrix
    assert add('grey_90x70', _photo(70, 90)[:, :, 0], quality=80)
    assert add('grey_8x8', _photo(8, 8, seed=16)[:, :, 0], quality=80)
    noise = np.random.default_rng(1).integers(0, 256, (41, 67, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:40, 0:64]
    check1 = (((yy + xx) & 1) * 255).astype(np.uint8)                         # black / white, one pixel
    yy, xx = np.mgrid[0:41, 0:67]
    check2 = np.where((((yy >> 1) + (xx >> 1)) & 1)[:, :, None] == 0, (255, 0, 0), (0, 255, 255)).astype(np.uint8)
    assert add('check1_grey', check1, quality=100)
    for sub in (0, 1, 2):
        assert add('noise_q100_s%d' % sub, noise, quality=100, subsampling=sub)
        assert add('noise_q30_s%d' % sub, noise, quality=30, subsampling=sub)
        assert add('check1_rgb_s%d' % sub, np.repeat(check1[:, :, None], 3, 2), quality=100, subsampling=sub)
        assert add('check2_s%d' % sub, check2, quality=100, subsampling=sub)
    counts = dict(matrix=matrix, images=len(images), luma=0, chroma=[0, 0, 0], full_blocks=0, entries=0)
    for im in images:
        nc = int(im.info['ncomp'][0])
        for c in range(nc):
            ac = im.plane_coef(c)[:, 1:]
            counts['entries'] += int(np.count_nonzero(ac))
            counts['full_blocks'] += int(np.count_nonzero(np.count_nonzero(ac, 1) == 63))
            if c == 0:
                counts['luma'] += _two_word(ac)
            else:
                counts['chroma'][im.sampling] += _two_word(ac)
    assert counts['luma'] >= 1 and min(counts['chroma']) >= 1 and counts['full_blocks'] >= 1, counts
    return tuple(images), counts


def _interleaved(n):
    """A fixed order in which neighbours differ in size, quality and sampling (the builder's order is sampling-major)."""
    step = next(s for s in range(n // 3 + 1, n) if np.gcd(s, n) == 1)
    return [(i * step) % n for i in range(n)]


def _index(name):
    return next(i for i, im in enumerate(_inputs()[0]) if im.name == name)


@functools.lru_cache(maxsize=4)
def _whole(index, flip):
    return preprocess_ref.preprocess_image(_inputs()[0][index].rgb, 256, 256, flip=bool(flip), oy=0, ox=0)


def _want(index, out, flip, oy, ox):
    """preprocess_image(PIL's pixels, out, out, flip, oy, ox): its crop comes after the resize and the flip and in front of an
    element-wise scale, so the window is cut from the whole 256 x 256 result (one resize per image and flip, not per window)."""
    return _whole(index, int(bool(flip)))[oy:oy + out, ox:ox + out]


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _to_dev(a):
    import torch
    return torch.from_numpy(_u8(a)).cuda()


def _filled(nbytes, byte):
    import torch
    return torch.full((int(nbytes),), byte, dtype=torch.uint8, device='cuda')


def _nan(*shape):
    import torch
    return torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')


def _desc(h, w, off, flip, oy, ox, resize=256):
    """comic_image_desc records filled as DevicePreprocessor._launch_split fills them."""
    from comic_amd import inputs
    h, w = np.asarray(h, np.int64), np.asarray(w, np.int64)
    desc = np.zeros(len(h), inputs.DevicePreprocessor._DESC_DTYPE)
    desc['offset'], desc['in_h'], desc['in_w'] = off, h, w
    desc['flip'], desc['oy'], desc['ox'] = flip, oy, ox
    desc['sy'] = (h / resize).astype(np.float32)
    desc['sx'] = (w / resize).astype(np.float32)
    return desc


def _submit_packed(paths):
    """comic_jpeg_pool_submit_packed + comic_jpeg_pool_wait of one batch, as JpegSplitPool does -> infos (coef_base assigned),
    status, the packed blob in use, samples of all planes."""
    lib = L.load_jpeg()
    n = len(paths)
    # room for everything: a block costs the file at least 4 bits (two codes) and the blob 3 units, an entry at least 3 bits
    # (a code and a value bit) and 1 unit, a two-word entry at least 12 bits -- 6 units per byte of file at the most
    cap = sum(8 * os.path.getsize(p) + 64 for p in paths)
    infos, status, blob = np.zeros(n, L.JPEG_INFO_DTYPE), np.full(n, 99, np.int32), np.zeros(cap, np.uint16)
    arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
    pool = lib.comic_jpeg_pool_create(3)
    assert pool
    try:
        h = lib.comic_jpeg_pool_submit_packed(pool, arr, n, infos.ctypes.data, status.ctypes.data, blob.ctypes.data, cap)
        used, planes = C.c_int64(-1), C.c_int64(-1)
        assert h and lib.comic_jpeg_pool_wait(pool, h, 60.0, C.byref(used), C.byref(planes)) == 0
    finally:
        lib.comic_jpeg_pool_destroy(pool)
    assert L.JPEG_TOO_SMALL not in status.tolist()
    return infos, status, blob[:used.value + (used.value & 1)].copy(), int(planes.value)


@pytest.fixture(scope='module')
def packed_set(tmp_path_factory):
    """The shared set as files, and as ONE packed batch of the decode pool (host side only)."""
    images, _ = _inputs()
    d = tmp_path_factory.mktemp('jpeg_set')
    paths = []
    for im in images:
        p = str(d / (im.name + '.jpg'))
        with open(p, 'wb') as f:
            f.write(im.data)
        paths.append(p)
    infos, status, blob, planes_total = _submit_packed(paths)
    assert (status == 0).all(), status
    for i, im in enumerate(images):
        assert infos['coef_count'][i] == im.info['coef_count'][0] and infos['coef_base'][i] % 64 == 0, im.name
    assert planes_total == sum(int(im.info['coef_count'][0]) for im in images)
    return dict(paths=paths, infos=infos, blob=blob, planes_total=planes_total)


@pytest.fixture(scope='module', autouse=True)
def _drop_the_set():
    yield
    _whole.cache_clear()
    _inputs.cache_clear()


def _run_packed(lib, blob_dev, infos, desc, planes_dev, out, out_hw, rgb_blob=None, entry='comic_jpeg_preprocess_packed'):
    import torch
    n = len(infos)
    dec = infos['ncomp'] > 0
    max_blocks = int(infos['coef_count'][dec].max()) // 64 if dec.any() else 0
    di, dd = _to_dev(infos), _to_dev(desc)
    L.check(getattr(lib, entry)(blob_dev.data_ptr(), di.data_ptr(), n, max_blocks, planes_dev.data_ptr(),
                                rgb_blob.data_ptr() if rgb_blob is not None else None, dd.data_ptr(), out.data_ptr(), out_hw,
                                out_hw, 256, L.stream_ptr()), entry)
    torch.cuda.synchronize()


def _first_diff(got, want):
    at = np.argwhere(got != want)
    return None if not len(at) else (tuple(int(v) for v in at[0]), got[tuple(at[0])], want[tuple(at[0])], len(at))


# ---- 1. comic_jpeg_pixels --------------------------------------------------------------------------------------------------
def test_device_pixels_equal_pil_over_the_whole_set():
    """One interleaved batch; two records in its middle have ncomp == 0 (their coefficients and pixel ranges are there: a kernel
    that ignored the flag would write).  The pixel blob starts as a sentinel: the 16-byte padding between images, the ranges of
    the two skipped records and a guard behind the last image must keep it."""
    import torch
    images, counts = _inputs()
    print('shared set:', counts)
    order = _interleaved(len(images))
    mid = len(order) // 2
    order[mid:mid] = [_index('photo_159x107_q85_s2'), _index('photo_83x125_q98_s0')]        # the two PIL-path records
    skipped = (mid, mid + 1)
    n = len(order)
    infos = np.concatenate([images[k].info for k in order])
    coef, base, off = [], 0, 0
    for j, k in enumerate(order):
        infos['coef_base'][j], infos['pixel_off'][j] = base, off
        coef.append(images[k].coef)
        base += images[k].coef.size
        off += (images[k].rgb.size + 15) // 16 * 16
    for j in skipped:
        infos['ncomp'][j] = 0
    dec = infos['ncomp'] > 0
    dev_coef = torch.from_numpy(np.concatenate(coef)).cuda()
    planes = _filled(base + GUARD, 0x5a)
    pixels = _filled(off + GUARD, 0xa5)
    dev_infos = _to_dev(infos)
    L.check(L.load().comic_jpeg_pixels(dev_coef.data_ptr(), dev_infos.data_ptr(), n, int(infos['coef_count'][dec].max()) // 64,
                                       int(infos['width'][dec].max()), int(infos['height'][dec].max()), planes.data_ptr(),
                                       pixels.data_ptr(), L.stream_ptr()), 'jpeg_pixels')
    torch.cuda.synchronize()
    got, end = pixels.cpu().numpy(), 0
    assert (planes.cpu().numpy()[base:] == 0x5a).all()
    for j, k in enumerate(order):
        im, o = images[k], int(infos['pixel_off'][j])
        assert (got[end:o] == 0xa5).all(), ('padding in front of', j, im.name)
        end = o + im.rgb.size
        if j in skipped:
            assert (got[o:end] == 0xa5).all(), ('a record with ncomp == 0 was written', j, im.name)
            continue
        px = got[o:end].reshape(im.rgb.shape)
        assert np.array_equal(px, im.rgb), (j, im.name, _first_diff(px, im.rgb))
    assert (got[end:] == 0xa5).all() and got.size - end >= GUARD


# ---- 2. planes of the packed kernel ----------------------------------------------------------------------------------------
def test_packed_planes_equal_the_dense_kernels_and_the_oracles(packed_set):
    """The packed form the pool made of the set and the dense coefficients of the same files, laid at the coef_base offsets the
    wait assigned, address the same plane layout: both inverse DCTs must fill [0, planes_total) with the oracle's planes over
    every component's whole padded block grid, and nothing behind it."""
    import torch
    images, _ = _inputs()
    lib = L.load()
    infos, total = packed_set['infos'], packed_set['planes_total']
    n = len(images)
    dense = np.zeros(total, np.int16)
    for i, im in enumerate(images):
        b = int(infos['coef_base'][i])
        dense[b:b + im.coef.size] = im.coef
    k = np.arange(n)
    desc = _desc(infos['height'], infos['width'], infos['pixel_off'], k % 2, (k * 7) % 33, (k * 5) % 33)
    pa, pb = _filled(total + GUARD, 0x00), _filled(total + GUARD, 0xff)
    oa, ob = _nan(n, 224, 224, 3), _nan(n, 224, 224, 3)
    _run_packed(lib, torch.from_numpy(packed_set['blob'].view(np.int16)).cuda(), infos, desc, pa, oa, 224)
    _run_packed(lib, torch.from_numpy(dense).cuda(), infos, desc, pb, ob, 224, entry='comic_jpeg_preprocess')
    ga, gb = pa.cpu().numpy(), pb.cpu().numpy()
    assert (ga[total:] == 0x00).all() and (gb[total:] == 0xff).all()
    for i, im in enumerate(images):
        rec, base = im.info[0], int(infos['coef_base'][i])
        for c in range(int(rec['ncomp'])):
            bh, bw = int(rec['blocks_h'][c]), int(rec['blocks_w'][c])
            want = jpeg_ref.idct_plane(im.plane_coef(c), rec['quant'][c].astype(np.int64), bh, bw)
            o = base + int(rec['coef_off'][c])
            for kind, g in (('packed', ga), ('dense', gb)):
                pl = g[o:o + want.size].reshape(want.shape)
                assert np.array_equal(pl, want), (kind, im.name, 'component', c, _first_diff(pl, want))
    assert np.array_equal(ga[:total], gb[:total])
    assert torch.equal(oa, ob) and not torch.isnan(oa).any()


# ---- 3. fused taps at the image borders ------------------------------------------------------------------------------------
@pytest.mark.parametrize('windows', ['whole_256', 'corners_224'])
def test_fused_taps_equal_the_oracle_at_the_image_borders(packed_set, windows):
    """whole_256: out == resize == 256 at offset 0, both flips -- no crop margin, so for an image of at most 256 pixels on a side
    every source row and column is a tap (partial MCUs, the copied / replicated ends of the fancy upsampling, the last odd row and
    column of 4:2:2 and 4:2:0); strips are upscaled, 256 x 256 is the identity (floor == ceil, weights 0).
    corners_224: the product's 224 window of the 256 resize at its four corner offsets, flips alternating.
    Every copy of an image has planes of its own; dst starts as NaN."""
    import torch
    images, _ = _inputs()
    n = len(images)
    if windows == 'whole_256':
        out_hw, cases = 256, [(flip, 0, 0) for flip in (0, 1)]
        params = [[case] * n for case in cases]
    else:
        out_hw = 224
        params = [[((i + c) % 2,) + CORNERS[c] for i in range(n)] for c in range(4)]
    copies = len(params)
    one, total = packed_set['infos'], packed_set['planes_total']
    infos = np.tile(one, copies)
    for c in range(copies):
        infos['coef_base'][c * n:(c + 1) * n] += c * total
    flat = [p for group in params for p in group]
    desc = _desc(infos['height'], infos['width'], infos['pixel_off'], [p[0] for p in flat], [p[1] for p in flat],
                 [p[2] for p in flat])
    planes = _filled(copies * total + GUARD, 0x77)
    out = _nan(copies * n, out_hw, out_hw, 3)
    _run_packed(L.load(), torch.from_numpy(packed_set['blob'].view(np.int16)).cuda(), infos, desc, planes, out, out_hw)
    got = out.cpu().numpy()
    assert (planes[copies * total:] == 0x77).all()
    for i in range(n):
        for j in range(i, copies * n, n):
            want = _want(i, out_hw, *flat[j])
            assert np.array_equal(got[j], want), (images[i].name, flat[j], _first_diff(got[j], want))


# ---- 4. batches with PIL-path images ---------------------------------------------------------------------------------------
def _corner_params(i):
    return ((i % 2,) + CORNERS[(i // 2) % 4])


def test_mixed_batch_leaves_the_decoded_neighbours_alone(packed_set, tmp_path):
    """A packed batch with a progressive JPEG and a PNG in its middle: the pool rejects both, and they travel as ncomp == 0 with
    PIL's RGB bytes in the blob (what _launch_split does).  Every image equals the oracle; the decoded ones equal what the same
    files give in a batch without the two, window for window (the corner windows of the test above)."""
    import torch
    from PIL import Image
    images, _ = _inputs()
    lib = L.load()
    pick = list(range(0, len(images), 5))
    prog, png = str(tmp_path / 'prog.jpg'), str(tmp_path / 'lossless.png')
    with open(prog, 'wb') as f:
        f.write(_encode(_photo(77, 101, seed=3), progressive=True, quality=85))
    Image.fromarray(_photo(120, 90, seed=9)).save(png)
    rejected = {prog: _pil(open(prog, 'rb').read()), png: np.asarray(Image.open(png).convert('RGB'))}
    src = [packed_set['paths'][k] for k in pick]
    at = len(src) // 2
    paths = src[:at] + [prog] + src[at:at + 1] + [png] + src[at + 1:]
    idx = pick[:at] + [None] + pick[at:at + 1] + [None] + pick[at + 1:]
    n = len(paths)
    infos, status, blob, total = _submit_packed(paths)
    assert status[at] == L.JPEG_UNSUPPORTED and status[at + 2] in (L.JPEG_UNSUPPORTED, L.JPEG_CORRUPT)
    assert all(status[j] == 0 for j in range(n) if idx[j] is not None)
    h, w, off = infos['height'].astype(np.int64), infos['width'].astype(np.int64), infos['pixel_off'].astype(np.int64)
    rgb, nbytes = [], 0
    for j in (at, at + 2):
        im = rejected[paths[j]]
        infos['ncomp'][j] = 0
        h[j], w[j], off[j] = im.shape[0], im.shape[1], nbytes
        rgb.append(im.reshape(-1))
        rgb.append(np.zeros(-im.size % 16, np.uint8))
        nbytes += (im.size + 15) // 16 * 16
    params = [_corner_params(j) for j in range(n)]
    desc = _desc(h, w, off, [p[0] for p in params], [p[1] for p in params], [p[2] for p in params])
    out = _nan(n, 224, 224, 3)
    _run_packed(lib, torch.from_numpy(blob.view(np.int16)).cuda(), infos, desc, _filled(total + GUARD, 0), out, 224,
                rgb_blob=torch.from_numpy(np.concatenate(rgb)).cuda())
    got = out.cpu().numpy()
    for j in range(n):
        if idx[j] is None:
            want = preprocess_ref.preprocess_image(rejected[paths[j]], 224, 224, bool(params[j][0]), params[j][1], params[j][2])
        else:
            want = _want(idx[j], 224, *params[j])
        assert np.array_equal(got[j], want), (paths[j], params[j], _first_diff(got[j], want))
    # the same decoded files, same windows, without the two rejected ones
    keep = [j for j in range(n) if idx[j] is not None]
    infos2, status2, blob2, total2 = _submit_packed([paths[j] for j in keep])
    assert (status2 == 0).all()
    out2 = _nan(len(keep), 224, 224, 3)
    _run_packed(lib, torch.from_numpy(blob2.view(np.int16)).cuda(), infos2, desc[keep], _filled(total2 + GUARD, 0xff), out2, 224)
    assert np.array_equal(out2.cpu().numpy(), got[keep])


@pytest.mark.parametrize('entry', ['comic_jpeg_preprocess', 'comic_jpeg_preprocess_packed'])
def test_pil_only_batch_skips_the_inverse_dct(entry):
    """Every image with ncomp == 0 and max_blocks == 0: no inverse DCT launch, the taps come from the RGB blob alone (the
    coefficient and plane buffers are never read: they hold a few bytes)."""
    import torch
    images, _ = _inputs()
    names = ('photo_100x1_q85_s0', 'photo_5x200_q35_s0', 'photo_17x9_q98_s2', 'photo_255x257_q85_s1', 'photo_8x8_q35_s0',
             'photo_161x3_q98_s1', 'photo_256x256_q35_s2', 'check2_s0')
    pick = [_index(name) for name in names]
    n = len(pick)
    infos = np.zeros(n, L.JPEG_INFO_DTYPE)
    rgb, offs, nbytes = [], [], 0
    for k in pick:
        im = images[k].rgb
        offs.append(nbytes)
        rgb += [im.reshape(-1), np.zeros(-im.size % 16, np.uint8)]
        nbytes += (im.size + 15) // 16 * 16
    params = [_corner_params(j + 1) for j in range(n)]
    desc = _desc([images[k].rgb.shape[0] for k in pick], [images[k].rgb.shape[1] for k in pick], offs, [p[0] for p in params],
                 [p[1] for p in params], [p[2] for p in params])
    out = _nan(n, 224, 224, 3)
    planes = _filled(64, 0x33)
    _run_packed(L.load(), torch.zeros(64, dtype=torch.int16, device='cuda'), infos, desc, planes, out, 224,
                rgb_blob=torch.from_numpy(np.concatenate(rgb)).cuda(), entry=entry)
    got = out.cpu().numpy()
    assert (planes.cpu().numpy() == 0x33).all()
    for j, k in enumerate(pick):
        want = _want(k, 224, *params[j])
        assert np.array_equal(got[j], want), (images[k].name, params[j], _first_diff(got[j], want))


# ---- 5. plane buffer reuse -------------------------------------------------------------------------------------------------
def test_a_batch_does_not_see_the_planes_of_the_batch_before(packed_set):
    """The loader keeps ONE coefficient, plane and output buffer for all batches (DevicePreprocessor._dev_planes): the small
    images, run where the large ones have just been, give the bits they give in fresh buffers."""
    import torch
    images, _ = _inputs()
    lib = L.load()
    big = [i for i, im in enumerate(images) if max(im.rgb.shape[:2]) >= 150]
    small = [i for i in range(len(images)) if i not in set(big)]
    assert len(big) >= 20 and len(small) >= 20
    runs = {}
    for name, pick in (('A', big), ('B', small)):
        infos, status, blob, total = _submit_packed([packed_set['paths'][i] for i in pick])
        assert (status == 0).all()
        params = [_corner_params(j) for j in range(len(pick))]
        desc = _desc(infos['height'], infos['width'], infos['pixel_off'], [p[0] for p in params], [p[1] for p in params],
                     [p[2] for p in params])
        runs[name] = (infos, blob.view(np.int16), total, desc)
    (ia, ba, ta, da), (ib, bb, tb, db) = runs['A'], runs['B']
    assert ta > tb
    coef = torch.zeros(max(ba.size, bb.size), dtype=torch.int16, device='cuda')
    planes = _filled(max(ta, tb) + GUARD, 0)
    out = _nan(max(len(ia), len(ib)), 224, 224, 3)
    coef[:ba.size].copy_(torch.from_numpy(ba))
    _run_packed(lib, coef, ia, da, planes, out, 224)
    coef[:bb.size].copy_(torch.from_numpy(bb))
    _run_packed(lib, coef, ib, db, planes, out, 224)
    fresh_planes, fresh_out = _filled(tb + GUARD, 0xff), _nan(len(ib), 224, 224, 3)
    _run_packed(lib, torch.from_numpy(bb).cuda(), ib, db, fresh_planes, fresh_out, 224)
    assert torch.equal(out[:len(ib)], fresh_out) and not torch.isnan(fresh_out).any()
    assert torch.equal(planes[:tb], fresh_planes[:tb])
    got = fresh_out.cpu().numpy()
    for j, k in enumerate(small):
        want = _want(k, 224, *_corner_params(j))
        assert np.array_equal(got[j], want), (images[k].name, _first_diff(got[j], want))
