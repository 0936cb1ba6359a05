"""Training augmentation of the input images: `--cnn_input_augment_crop area` and `--cnn_input_augment_color fast|full`.

slim's `distorted_bounding_box_crop` and `distort_color`, which the reference carries and `preprocess_for_train` never calls
(common/inputs/preprocessing/inception_preprocessing_radix.py:45-156 beside :158-234).  The definition of the pixel
arithmetic is include/comic_hip.h's (comic_image_aug); the device computes it inside the preprocessing launches
(csrc/augment_dev.h), `apply` below is the same in numpy for the host loader path, bit for bit.

The loader's producer thread draws ONE 64-bit key per image; everything else is `augment_params`, a pure function of the
keys and the image sizes, evaluated where the sizes are known -- so the augmentation is a function of the seed and the
sample order on every loader path."""
import numpy as np

from . import _lib as L

CROPS = ('fixed', 'area')
COLORS = ('none', 'fast', 'full')
AREA_MIN_DEFAULT = 0.35
FLAGS = ('cnn_input_augment_crop', 'cnn_input_augment_color', 'cnn_input_augment_area_min')
B, S, H, C = L.AUG_OP_BRIGHTNESS, L.AUG_OP_SATURATION, L.AUG_OP_HUE, L.AUG_OP_CONTRAST
# slim's orderings (distort_color, :66-113)
ORDERINGS = {'none': ((0, 0, 0, 0),),
             'fast': ((B, S, 0, 0), (S, B, 0, 0)),
             'full': ((B, S, H, C), (S, B, C, H), (C, H, B, S), (H, S, C, B))}
MAX_DELTA_BRIGHTNESS, MAX_DELTA_HUE = 32.0 / 255.0, 0.2
FACTOR_LOW, FACTOR_HIGH = 0.5, 1.5            # saturation and contrast
ASPECT_LOW, ASPECT_HIGH = 3.0 / 4.0, 4.0 / 3.0
ATTEMPTS = 10
# positions in a key's counter stream
DRAW_FLIP, DRAW_OY, DRAW_OX, DRAW_ORDER, DRAW_BRIGHTNESS, DRAW_SATURATION, DRAW_HUE, DRAW_CONTRAST, DRAW_BOX = range(9)


class AugmentSpec(object):
    """The three flags and the geometry they act in."""

    def __init__(self, crop='fixed', color='none', area_min=AREA_MIN_DEFAULT, out_h=224, out_w=224, resize=256):
        crop, color = crop or 'fixed', color or 'none'
        if crop not in CROPS:
            raise ValueError('--cnn_input_augment_crop must be one of %s, got %r' % (CROPS, crop))
        if color not in COLORS:
            raise ValueError('--cnn_input_augment_color must be one of %s, got %r' % (COLORS, color))
        area_min = float(area_min)
        if not 0.0 < area_min <= 1.0:
            raise ValueError('--cnn_input_augment_area_min must lie in (0, 1], got %r' % (area_min,))
        self.crop, self.color, self.area_min = crop, color, area_min
        self.out_h, self.out_w, self.resize = int(out_h), int(out_w), int(resize)

    @property
    def active(self):
        return self.crop != 'fixed' or self.color != 'none'


def spec_from_config(c):
    """The AugmentSpec of a configuration, None with the flags at their defaults (their keys are then absent)."""
    h, w = c.cnn_input_size
    spec = AugmentSpec(getattr(c, 'cnn_input_augment_crop', None), getattr(c, 'cnn_input_augment_color', None),
                       getattr(c, 'cnn_input_augment_area_min', AREA_MIN_DEFAULT), h, w)
    return spec if spec.active else None


def refuse_bad_options(kw):
    """Values out of range, and any of the flags with --cnn_input_augment False.  Called before anything touches the GPU."""
    crop = kw.get('cnn_input_augment_crop') or 'fixed'
    color = kw.get('cnn_input_augment_color') or 'none'
    area_min = kw.get('cnn_input_augment_area_min', AREA_MIN_DEFAULT)
    area_min = AREA_MIN_DEFAULT if area_min is None else area_min
    spec = AugmentSpec(crop, color, area_min)
    given = spec.active or float(area_min) != AREA_MIN_DEFAULT
    if given and not kw.get('cnn_input_augment', True):
        raise ValueError('--cnn_input_augment_crop / _color / _area_min need --cnn_input_augment True')
    if float(area_min) != AREA_MIN_DEFAULT and crop != 'area':
        raise ValueError('--cnn_input_augment_area_min needs --cnn_input_augment_crop area')


def dir_suffix(args):
    """'_augA0.35' for the area crop (with its smallest area share), '_augCfull' / '_augCfast' for the colour distortion,
    '_augA0.35Cfull' for both; '' with the flags at their defaults."""
    crop = getattr(args, 'cnn_input_augment_crop', None) or 'fixed'
    color = getattr(args, 'cnn_input_augment_color', None) or 'none'
    out = ''
    if crop == 'area':
        out += 'A%g' % float(getattr(args, 'cnn_input_augment_area_min', AREA_MIN_DEFAULT))
    if color != 'none':
        out += 'C' + color
    return '_aug' + out if out else ''


def pop_defaults(kwargs):
    """Flags at their defaults leave the configuration: it is the one of a run without them."""
    if (kwargs.get('cnn_input_augment_crop') or 'fixed') == 'fixed':
        kwargs.pop('cnn_input_augment_crop', None)
        kwargs.pop('cnn_input_augment_area_min', None)
    if (kwargs.get('cnn_input_augment_color') or 'none') == 'none':
        kwargs.pop('cnn_input_augment_color', None)


# ---- the draws ---------------------------------------------------------------------------------------------------------------
_GAMMA = np.uint64(0x9E3779B97F4A7C15)


def splitmix64(z):
    """csrc/splitmix.h on uint64 arrays."""
    with np.errstate(over='ignore'):
        z = np.asarray(z, np.uint64) + _GAMMA
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniform(keys, j):
    """Draw j of every key's counter stream (splitmix64 of key + j * gamma), as a float64 in [0, 1)."""
    with np.errstate(over='ignore'):
        x = splitmix64(np.asarray(keys, np.uint64) + np.uint64(j) * _GAMMA)
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


class AugmentParams(object):
    """Of one batch: `aug` (comic_image_aug records, _lib.IMAGE_AUG_DTYPE), `flip`, `oy`, `ox` (for comic_image_desc) and
    whether any record holds a contrast op (a second pass)."""
    __slots__ = ('aug', 'flip', 'oy', 'ox', 'contrast')

    def __init__(self, aug, flip, oy, ox):
        self.aug, self.flip, self.oy, self.ox = aug, flip, oy, ox
        self.contrast = bool((aug['ops'] == C).any())


def draw_boxes(keys, in_h, in_w, area_min):
    """torchvision's RandomResizedCrop rule -> (cy, cx, ch, cw, fallback).  Up to 10 attempts: area = U[area_min, 1] H W,
    aspect log-uniform in [3/4, 4/3], w = round(sqrt(area * aspect)), h = round(sqrt(area / aspect)), taken when
    1 <= w <= W and 1 <= h <= H with a uniform origin; else the centred largest box whose aspect lies in the range."""
    keys = np.asarray(keys, np.uint64)
    Hh, Ww = np.asarray(in_h, np.int64), np.asarray(in_w, np.int64)
    j = DRAW_BOX + 4 * np.arange(ATTEMPTS, dtype=np.uint64)
    with np.errstate(over='ignore'):
        k = keys[:, None] + j[None, :] * _GAMMA                            # [n, attempts]: the attempt's first counter
        u = [(splitmix64(k + np.uint64(d) * _GAMMA) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 for d in range(4)]
    area = (area_min + u[0] * (1.0 - area_min)) * (Hh * Ww)[:, None]
    aspect = np.exp(np.log(ASPECT_LOW) + u[1] * (np.log(ASPECT_HIGH) - np.log(ASPECT_LOW)))
    w = np.rint(np.sqrt(area * aspect)).astype(np.int64)
    h = np.rint(np.sqrt(area / aspect)).astype(np.int64)
    ok = (w >= 1) & (w <= Ww[:, None]) & (h >= 1) & (h <= Hh[:, None])
    first = np.argmax(ok, axis=1)
    rows = np.arange(len(keys))
    fallback = ~ok[rows, first]
    ch, cw = h[rows, first], w[rows, first]
    cy = np.floor(u[2][rows, first] * (Hh - ch + 1)).astype(np.int64)
    cx = np.floor(u[3][rows, first] * (Ww - cw + 1)).astype(np.int64)
    ratio = Ww / Hh
    fw = np.where(ratio > ASPECT_HIGH, np.rint(Hh * ASPECT_HIGH).astype(np.int64), Ww)
    fh = np.where(ratio < ASPECT_LOW, np.rint(Ww / ASPECT_LOW).astype(np.int64), Hh)
    fw, fh = np.clip(fw, 1, Ww), np.clip(fh, 1, Hh)
    ch, cw = np.where(fallback, fh, ch), np.where(fallback, fw, cw)
    cy, cx = np.where(fallback, (Hh - fh) // 2, cy), np.where(fallback, (Ww - fw) // 2, cx)
    return cy, cx, ch, cw, fallback


def augment_params(keys, in_h, in_w, spec):
    """keys [n] uint64, the images' sizes -> AugmentParams.  Pure and vectorised over the batch."""
    keys = np.asarray(keys, np.uint64)
    in_h, in_w = np.asarray(in_h, np.int64), np.asarray(in_w, np.int64)
    n = len(keys)
    aug = np.zeros(n, L.IMAGE_AUG_DTYPE)
    flip = uniform(keys, DRAW_FLIP) < 0.5
    oy = np.floor(uniform(keys, DRAW_OY) * (spec.resize - spec.out_h + 1)).astype(np.int64)
    ox = np.floor(uniform(keys, DRAW_OX) * (spec.resize - spec.out_w + 1)).astype(np.int64)
    if spec.crop == 'area':
        cy, cx, ch, cw, _ = draw_boxes(keys, in_h, in_w, spec.area_min)
        aug['mode'] = L.AUG_BOX
        aug['cy'], aug['cx'], aug['ch'], aug['cw'] = cy, cx, ch, cw
        aug['sy'] = (ch / spec.out_h).astype(np.float32)
        aug['sx'] = (cw / spec.out_w).astype(np.float32)
        oy, ox = np.zeros(n, np.int64), np.zeros(n, np.int64)
    orders = np.array(ORDERINGS[spec.color], np.uint8)
    aug['ops'] = orders[np.floor(uniform(keys, DRAW_ORDER) * len(orders)).astype(np.int64)]
    if spec.color != 'none':
        aug['brightness'] = ((2.0 * uniform(keys, DRAW_BRIGHTNESS) - 1.0) * MAX_DELTA_BRIGHTNESS).astype(np.float32)
        aug['saturation'] = (FACTOR_LOW + uniform(keys, DRAW_SATURATION) * (FACTOR_HIGH - FACTOR_LOW)).astype(np.float32)
    if spec.color == 'full':
        aug['hue'] = ((2.0 * uniform(keys, DRAW_HUE) - 1.0) * MAX_DELTA_HUE).astype(np.float32)
        aug['contrast'] = (FACTOR_LOW + uniform(keys, DRAW_CONTRAST) * (FACTOR_HIGH - FACTOR_LOW)).astype(np.float32)
    return AugmentParams(aug, flip, oy, ox)


# ---- the pixel arithmetic in numpy (host loader path) --------------------------------------------------------------------------
_f = np.float32


def _wrap01(t):
    f = t - np.floor(t)
    return np.where(f >= _f(1), _f(0), f).astype(np.float32)


def rgb_to_hsv(c):
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    d = mx - mn
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(mx > 0, d / mx, _f(0)).astype(np.float32)
        hr, hg, hb = (g - b) / d, _f(2) + (b - r) / d, _f(4) + (r - g) / d
    hh = np.where(d == 0, _f(0), np.where(mx == r, hr, np.where(mx == g, hg, hb))).astype(np.float32)
    return _wrap01(hh * _f(1.0 / 6)), s, mx


def hsv_to_rgb(h, s, v):
    h6, vs = h * _f(6), v * s
    out = []
    for n in (5, 3, 1):
        t = _f(n) + h6
        k = np.where(t >= _f(6), t - _f(6), t)
        m = np.minimum(np.maximum(np.minimum(k, _f(4) - k), _f(0)), _f(1))
        out.append(v - vs * m)
    return np.stack(out, -1).astype(np.float32)


def fixed_sums(c):
    """per channel: the int64 sum of rint(double(v) * 2^32) over the pixels"""
    return np.rint(c.astype(np.float64) * 4294967296.0).astype(np.int64).reshape(-1, 3).sum(0)


def distort_color(c, rec):
    """The record's ops on the [0,1] pixels c [h, w, 3] float32, then the clamp (where there is an op)."""
    ops = [int(o) for o in rec['ops'] if int(o) != L.AUG_OP_NONE]
    for op in ops:
        if op == B:
            c = c + _f(rec['brightness'])
        elif op == S:
            h, s, v = rgb_to_hsv(c)
            c = hsv_to_rgb(h, np.minimum(np.maximum(s * _f(rec['saturation']), _f(0)), _f(1)), v)
        elif op == H:
            h, s, v = rgb_to_hsv(c)
            c = hsv_to_rgb(_wrap01(h + _f(rec['hue'])), s, v)
        elif op == C:
            mean = (fixed_sums(c).astype(np.float64) / (4294967296.0 * (c.shape[0] * c.shape[1]))).astype(np.float32)
            c = (c - mean) * _f(rec['contrast']) + mean
    if ops:
        c = np.minimum(np.maximum(c, _f(0)), _f(1))
    return c.astype(np.float32)
