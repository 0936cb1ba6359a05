"""The training augmentations of include/comic_hip.h (comic_image_aug) restated in plain numpy: float32 at the definition's
rounding points, int64 sums for the contrast mean -- the reference the device kernels and the host loader path are compared
with bit for bit -- and the loader's draw rule (one key per image -> box, ordering, parameters) restated one key at a time on
Python integers, independently of comic_amd.augment's vectorised form.

Not derived from the code under test: the geometry is tf.image.resize_bilinear (align_corners=False) of the cropped
tensor, the colour ops are slim's distort_color with the HSV formulas written out operation by operation below."""
import numpy as np

f32 = np.float32
NONE, BRIGHTNESS, SATURATION, HUE, CONTRAST = 0, 1, 2, 3, 4
LEGACY, BOX = 0, 1
ORDERINGS = {'none': [[0, 0, 0, 0]],
             'fast': [[BRIGHTNESS, SATURATION, 0, 0], [SATURATION, BRIGHTNESS, 0, 0]],
             'full': [[BRIGHTNESS, SATURATION, HUE, CONTRAST], [SATURATION, BRIGHTNESS, CONTRAST, HUE],
                      [CONTRAST, HUE, BRIGHTNESS, SATURATION], [HUE, SATURATION, CONTRAST, BRIGHTNESS]]}
AUG_DTYPE = np.dtype([('mode', '<i4'), ('cy', '<i4'), ('cx', '<i4'), ('ch', '<i4'), ('cw', '<i4'), ('sy', '<f4'), ('sx', '<f4'),
                      ('ops', 'u1', 4), ('brightness', '<f4'), ('saturation', '<f4'), ('hue', '<f4'), ('contrast', '<f4')])


def record(mode=LEGACY, box=(0, 0, 1, 1), out_hw=(1, 1), ops=(), brightness=0.0, saturation=1.0, hue=0.0, contrast=1.0):
    r = np.zeros((), AUG_DTYPE)
    r['mode'] = mode
    r['cy'], r['cx'], r['ch'], r['cw'] = box
    r['sy'], r['sx'] = f32(box[2] / out_hw[0]), f32(box[3] / out_hw[1])
    r['ops'] = list(ops) + [0] * (4 - len(ops))
    r['brightness'], r['saturation'], r['hue'], r['contrast'] = brightness, saturation, hue, contrast
    return r


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def _lerp(a, b, w):
    d = (b - a).astype(f32)
    m = (d * w).astype(f32)
    return (a + m).astype(f32)


def _bilinear(src01, rows, cols, limit_h, limit_w, origin):
    """src01 [H, W, 3] float32 in [0,1]; rows / cols: float32 source coordinates relative to `origin`; the upper taps clamp at
    limit - 1 (relative)."""
    y0 = np.floor(rows).astype(np.int64)
    x0 = np.floor(cols).astype(np.int64)
    y1 = np.minimum(np.ceil(rows).astype(np.int64), limit_h - 1)
    x1 = np.minimum(np.ceil(cols).astype(np.int64), limit_w - 1)
    wy = (rows - y0.astype(f32)).astype(f32)[:, None, None]
    wx = (cols - x0.astype(f32)).astype(f32)[None, :, None]
    oy, ox = origin
    tl, tr = src01[oy + y0][:, ox + x0], src01[oy + y0][:, ox + x1]
    bl, br = src01[oy + y1][:, ox + x0], src01[oy + y1][:, ox + x1]
    return _lerp(_lerp(tl, tr, wx), _lerp(bl, br, wx), wy)


def geometry(rgb_u8, out_h, out_w, flip, rec, oy=0, ox=0, resize=256):
    """uint8 [H, W, 3] -> the [0,1] float32 pixels [out_h, out_w, 3] in front of the colour ops."""
    src = (rgb_u8.astype(f32) * f32(1.0 / 255)).astype(f32)
    in_h, in_w = rgb_u8.shape[:2]
    if int(rec['mode']) == BOX:
        cy, cx, ch, cw = int(rec['cy']), int(rec['cx']), int(rec['ch']), int(rec['cw'])
        assert 0 <= cy and cy + ch <= in_h and 0 <= cx and cx + cw <= in_w and ch >= 1 and cw >= 1
        xs = np.arange(out_w)
        if flip:
            xs = out_w - 1 - xs
        rows = (np.arange(out_h).astype(f32) * f32(rec['sy'])).astype(f32)
        cols = (xs.astype(f32) * f32(rec['sx'])).astype(f32)
        return _bilinear(src, rows, cols, ch, cw, (cy, cx))
    ys = oy + np.arange(out_h)
    xs = ox + np.arange(out_w)
    if flip:
        xs = resize - 1 - xs
    rows = (ys.astype(f32) * f32(in_h / resize)).astype(f32)
    cols = (xs.astype(f32) * f32(in_w / resize)).astype(f32)
    return _bilinear(src, rows, cols, in_h, in_w, (0, 0))


# ---- colour ----------------------------------------------------------------------------------------------------------------------
def wrap01(t):
    """t - floor(t); 0 where the subtraction rounds up to 1"""
    t = np.asarray(t, f32)
    fr = (t - np.floor(t)).astype(f32)
    fr[fr >= f32(1)] = f32(0)
    return fr


def rgb_to_hsv(c):
    """v = max; d = max - min; s = d / v, 0 where v <= 0; h = 0 at d = 0, else by the channel holding the maximum -- red before
    green before blue where maxima tie -- (g - b) / d, 2 + (b - r) / d, 4 + (r - g) / d; times float32(1/6); wrapped into [0,1)."""
    c = np.asarray(c, f32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    v = c.max(-1)
    d = (v - c.min(-1)).astype(f32)
    s = np.zeros_like(v)
    pos = v > 0
    s[pos] = (d[pos] / v[pos]).astype(f32)
    hh = np.zeros_like(v)
    col = d != 0
    is_r = col & (v == r)
    is_g = col & ~is_r & (v == g)
    is_b = col & ~is_r & ~is_g
    hh[is_r] = ((g - b)[is_r].astype(f32) / d[is_r]).astype(f32)
    hh[is_g] = (f32(2) + ((b - r)[is_g].astype(f32) / d[is_g]).astype(f32)).astype(f32)
    hh[is_b] = (f32(4) + ((r - g)[is_b].astype(f32) / d[is_b]).astype(f32)).astype(f32)
    return wrap01((hh * f32(1.0 / 6)).astype(f32)), s, v


def hsv_to_rgb(h, s, v):
    """channel n of (5, 3, 1) for (r, g, b): k = n + 6h, less 6 where >= 6; v - (v s) clamp(min(k, 4 - k), 0, 1)"""
    h6 = (np.asarray(h, f32) * f32(6)).astype(f32)
    vs = (np.asarray(v, f32) * np.asarray(s, f32)).astype(f32)
    out = np.empty(h6.shape + (3,), f32)
    for i, n in enumerate((5.0, 3.0, 1.0)):
        k = (f32(n) + h6).astype(f32)
        big = k >= f32(6)
        k[big] = (k[big] - f32(6)).astype(f32)
        m = np.clip(np.minimum(k, (f32(4) - k).astype(f32)), f32(0), f32(1)).astype(f32)
        out[..., i] = (v - (vs * m).astype(f32)).astype(f32)
    return out


def brightness(c, delta):
    return (np.asarray(c, f32) + f32(delta)).astype(f32)


def saturation(c, factor):
    h, s, v = rgb_to_hsv(c)
    return hsv_to_rgb(h, np.clip((s * f32(factor)).astype(f32), f32(0), f32(1)), v)


def hue(c, delta):
    h, s, v = rgb_to_hsv(c)
    return hsv_to_rgb(wrap01((h + f32(delta)).astype(f32)), s, v)


def channel_sums(c):
    """int64 per channel: every pixel contributes rint(double(v) * 2^32)"""
    q = np.rint(np.asarray(c, f32).astype(np.float64) * 4294967296.0).astype(np.int64)
    return q.reshape(-1, 3).sum(axis=0, dtype=np.int64)


def contrast(c, factor):
    c = np.asarray(c, f32)
    n = c.size // 3
    mean = (channel_sums(c).astype(np.float64) / (4294967296.0 * n)).astype(f32)
    return (((c - mean).astype(f32) * f32(factor)).astype(f32) + mean).astype(f32)


def distort(c, rec):
    """the record's ops in order on the [0,1] pixels of ONE image (the contrast mean is the image's), the final clamp where
    there was an op"""
    any_op = False
    for op in [int(o) for o in rec['ops']]:
        if op == NONE:
            continue
        any_op = True
        c = {BRIGHTNESS: lambda a: brightness(a, rec['brightness']), SATURATION: lambda a: saturation(a, rec['saturation']),
             HUE: lambda a: hue(a, rec['hue']), CONTRAST: lambda a: contrast(a, rec['contrast'])}[op](c)
    if any_op:
        c = np.clip(c, f32(0), f32(1)).astype(f32)
    return c


def preprocess(rgb_u8, out_h, out_w, flip, rec, oy=0, ox=0, resize=256):
    """The network input of one image: geometry, colour ops, (v - 0.5) * 2."""
    c = distort(geometry(rgb_u8, out_h, out_w, flip, rec, oy, ox, resize), rec)
    return ((c - f32(0.5)).astype(f32) * f32(2)).astype(f32)


# ---- the draw rule, one key at a time ---------------------------------------------------------------------------------------------
MASK = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


def splitmix64(z):
    z = (z + GAMMA) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def u01(key, j):
    """draw j of the key's counter stream: the top 53 bits of splitmix64(key + j * gamma) as a float64 in [0, 1)"""
    return (splitmix64((int(key) + j * GAMMA) & MASK) >> 11) * 2.0 ** -53


def expected_box(key, H, W, area_min):
    """-> (cy, cx, ch, cw, fallback): draws 8 + 4a .. 11 + 4a of attempt a are area, aspect, origin y, origin x"""
    lo, hi = 3.0 / 4.0, 4.0 / 3.0
    for a in range(10):
        area = (area_min + u01(key, 8 + 4 * a) * (1.0 - area_min)) * (H * W)
        ar = float(np.exp(np.log(lo) + u01(key, 9 + 4 * a) * (np.log(hi) - np.log(lo))))
        w = int(np.rint(np.sqrt(area * ar)))
        h = int(np.rint(np.sqrt(area / ar)))
        if 1 <= w <= W and 1 <= h <= H:
            return (int(np.floor(u01(key, 10 + 4 * a) * (H - h + 1))), int(np.floor(u01(key, 11 + 4 * a) * (W - w + 1))), h, w,
                    False)
    h, w = H, W
    if W / H < lo:
        h = min(max(int(np.rint(W / lo)), 1), H)
    elif W / H > hi:
        w = min(max(int(np.rint(H * hi)), 1), W)
    return (H - h) // 2, (W - w) // 2, h, w, True


def expected_params(key, H, W, crop, color, area_min, out_h, out_w, resize=256):
    """-> (record, flip, oy, ox) of one key: draw 0 flip, 1 / 2 the window of the fixed crop, 3 the ordering, 4 .. 7 brightness,
    saturation, hue, contrast"""
    flip = u01(key, 0) < 0.5
    oy = int(np.floor(u01(key, 1) * (resize - out_h + 1)))
    ox = int(np.floor(u01(key, 2) * (resize - out_w + 1)))
    r = np.zeros((), AUG_DTYPE)
    if crop == 'area':
        cy, cx, ch, cw, _ = expected_box(key, H, W, area_min)
        r['mode'] = BOX
        r['cy'], r['cx'], r['ch'], r['cw'] = cy, cx, ch, cw
        r['sy'], r['sx'] = f32(ch / out_h), f32(cw / out_w)
        oy = ox = 0
    orders = ORDERINGS[color]
    r['ops'] = orders[int(np.floor(u01(key, 3) * len(orders)))]
    if color != 'none':
        r['brightness'] = f32((2.0 * u01(key, 4) - 1.0) * (32.0 / 255.0))
        r['saturation'] = f32(0.5 + u01(key, 5) * 1.0)
    if color == 'full':
        r['hue'] = f32((2.0 * u01(key, 6) - 1.0) * 0.2)
        r['contrast'] = f32(0.5 + u01(key, 7) * 1.0)
    return r, bool(flip), oy, ox
