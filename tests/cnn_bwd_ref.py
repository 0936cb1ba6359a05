"""Float64 references of the CNN backward kernels (csrc/conv_bwd.hip), each on the operands ONE launch reads, and the seeded
operand builders and case tables that tests/test_cnn_bwd_ref_cpu.py and tests/test_gpu_cnn_bwd_ops.py share.  numpy only.

The backward of a conv reads (x, y, dy, scale, w_master); y is GIVEN here, not computed by a forward, so no ReLU mask or pool
arg-max can differ between the device and the reference and every launch is held to the accuracy of its own arithmetic:

  act_grad        dz = store(fl32(1[y > 0] dy scale)) bit for bit (zero-dilated for stride 2), d beta = sum 1[y > 0] dy
  conv_wgrad      dw[co][k] = sum_pixels dz[p][co] xcol[p][k] from the STORED dz, k = (kh KW + kw) Cin + ci
  pack_bwd        the backward-data filter [Cin][Kpad2] bit for bit (flipped taps)
  conv_dgrad      gx += the transposed convolution of the stored dz with the packed filter
  *_pool_grad     max: the first maximum in (kh, kw) scan order, strict >, out-of-image taps -inf; avg: / valid taps
  fused_act_grad  the producer's activation gradient applied to fp32 backward-data accumulators

Plans: 'f32', 'bf16' and 'x3' (bf16 buffers of three channel regions [hi | lo | hi], fp32 gradient buffers).  Values travel as
float32 arrays (a bf16 value is a float32 whose low 16 bits are zero); bit-exact comparisons look at bits(), which tells -0.0
from 0.0."""
import collections
import math

import numpy as np

PLANS = ('f32', 'bf16', 'x3')
# bars of the op tests whose arithmetic the launches share (tests/test_gpu_ops.py): fp32-accumulated products of exactly
# representable operands (test_gemm_f32), the three-product x3 forms that omit lo*lo (test_gemm_f32_split3) and bf16 stores
# (test_conv_bn_relu: max-norm 1e-2 against the bf16-rounded expectation)
F32_BAR, X3_BAR, BF16_STORE_BAR = 1e-5, 5e-5, 1e-2
BF16_MIN_NORMAL = np.float32(2.0 ** -126)

Geo = collections.namedtuple('Geo', 'B H W Cin Cout KH KW S PT PL Ho Wo')


def geo(B, H, W, Cin, Cout, k, s=1, pad='VALID'):
    """pad: 'VALID', 'SAME' (TensorFlow's: the smaller half on top / left) or an explicit (PT, PL) with the same padding below"""
    kh, kw = (k, k) if isinstance(k, int) else k

    def one(n, kk, p):
        if p == 'VALID':
            return (n - kk) // s + 1, 0
        if p == 'SAME':
            out = -(-n // s)
            return out, max((out - 1) * s + kk - n, 0) // 2
        return (n + 2 * p - kk) // s + 1, p
    ph, pw = (pad, pad) if isinstance(pad, str) else pad
    Ho, pt = one(H, kh, ph)
    Wo, pl = one(W, kw, pw)
    return Geo(B, H, W, Cin, Cout, kh, kw, s, pt, pl, Ho, Wo)


def kpad(k):
    return (k + 63) // 64 * 64


# ----------------------------------------------------------------------------------------------- number formats -------
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bf16_round(x):
    """float32 -> bf16, round to nearest even, as float32 (finite inputs)"""
    u = bits(x)
    return ((u + (((u >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)).view(np.float32)


def split3(v):
    """v -> hi = bf16(v), lo = bf16(v - hi) (float32 subtraction, exact)"""
    v = np.asarray(v, np.float32)
    hi = bf16_round(v)
    return hi, bf16_round(v - hi)


def regions(hi, lo):
    """[hi | lo | hi] along the channel axis"""
    return np.concatenate([hi, lo, hi], -1)


def store(v, plan):
    """a float32 value as the plan stores it in an activation-sized buffer (x3: the regions)"""
    v = np.asarray(v, np.float32)
    if plan == 'f32':
        return v
    if plan == 'bf16':
        return bf16_round(v)
    return regions(*split3(v))


def representable(v, plan):
    """the nearest value the plan's storage holds (x3: hi + lo, exact in float32; store() of it sums back to it)"""
    v = np.asarray(v, np.float32)
    if plan == 'bf16':
        return bf16_round(v)
    if plan == 'x3':
        hi, lo = split3(v)
        return np.where(lo == 0, hi, hi + lo)          # (keeps the sign of -0.0)
    return v


def logical(a, plan, dtype=np.float64):
    """the value a stored tensor stands for (x3: hi + lo)"""
    a = np.asarray(a, dtype)
    if plan != 'x3':
        return a
    c = a.shape[-1] // 3
    return a[..., :c] + a[..., c:2 * c]


# ----------------------------------------------------------------------------------------------- operand builders ----
def _rng(*key):
    return np.random.default_rng([int(k) & 0x7FFFFFFF for k in key])


def make_y(seed, shape, plan):
    """forward output as the backward reads it: N(0, 1), so about half of it is <= 0, with exact 0.0, -0.0 and the smallest
    positive bf16 normal planted in front; representable in the storage type.  -> logical float32 values (x3: hi + lo)"""
    y = _rng(seed, 1).standard_normal(shape).astype(np.float32)
    flat = y.reshape(-1)
    flat[0], flat[1], flat[2], flat[3] = 0.0, -0.0, BF16_MIN_NORMAL, -BF16_MIN_NORMAL
    return representable(y, plan)


def make_dy(seed, shape, plan, scale=1.0):
    """gradient of the output with a non-zero mean (a zero-mean sum is a sqrt(N)-sized random number: the masks a kernel gets
    wrong would hide in it; see _seeds of tests/test_gpu_path.py)"""
    g = ((1 + 0.5 * _rng(seed, 2).standard_normal(shape)) * scale).astype(np.float32)
    return bf16_round(g) if plan == 'bf16' else g


def make_x(seed, shape, plan):
    return representable(_rng(seed, 3).standard_normal(shape).astype(np.float32), plan)


def make_scale(seed, C):
    return _rng(seed, 4).uniform(0.5, 1.5, C).astype(np.float32)


def make_master(seed, g):
    """fp32 master filter [Cout][Kpad], k = (kh KW + kw) Cin + ci, zero padding columns"""
    K = g.KH * g.KW * g.Cin
    w = np.zeros((g.Cout, kpad(K)), np.float32)
    w[:, :K] = _rng(seed, 5).standard_normal((g.Cout, K)) / math.sqrt(K)
    return w


def prefill(seed, shape, plan_dtype='f32', lo=0.25, hi=0.75):
    """known non-zero values for a buffer a launch accumulates into"""
    v = _rng(seed, 6).uniform(lo, hi, shape).astype(np.float32)
    return bf16_round(v) if plan_dtype == 'bf16' else v


def tie_map(seed, shape):
    """max-pool input drawn from 8 distinct bf16 values and ReLU zeros, the largest value the most frequent one: most windows
    have tied maxima (and the ties are between non-zero values, whose gradient no ReLU mask hides)"""
    vals = np.array([0.0, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 2.5, 3.0], np.float32)
    prob = [0.2] + [0.05] * 7 + [0.45]
    return vals[_rng(seed, 7).choice(len(vals), shape, p=prob)]


# ----------------------------------------------------------------------------------------------- references ----------
def dilate(v, S):
    """[B, Ho, Wo, C] -> [B, (Ho-1) S + 1, (Wo-1) S + 1, C] with zeros between the pixels"""
    if S == 1:
        return v
    B, Ho, Wo, C = v.shape
    out = np.zeros((B, (Ho - 1) * S + 1, (Wo - 1) * S + 1, C), v.dtype)
    out[:, ::S, ::S] = v
    return out


def act_grad(y, dy, scale, dtype, S=1):
    """y, dy [B, Ho, Wo, C] float32 (logical values), scale [C] -> (dz, dbeta): dz the float32 values of the stored d-conv
    tensor in the device layout ('x3': [hi | lo | hi]; stride S: zero-dilated), dbeta float64 [C], unscaled"""
    y, dy, scale = np.asarray(y, np.float32), np.asarray(dy, np.float32), np.asarray(scale, np.float32)
    g = np.where(y > 0, dy, np.float32(0))
    z = g * scale                                    # one float32 product
    return dilate(store(z, dtype), S), g.astype(np.float64).sum((0, 1, 2))


def fused_act_grad(g, y_p, scale_p, dtype='bf16'):
    """g [B, H, W, C]: the fp32 accumulators of a backward-data launch (the gradient at the producer's output) ->
    (dz_p, dbeta_p) as the fused epilogue leaves them: dz_p = store(fl32(g 1[y_p > 0]) scale_p), dbeta_p = sum g 1[y_p > 0]"""
    return act_grad(y_p, g, scale_p, dtype)


def im2col(x, g, dtype=np.float64):
    """[B, H, W, Cin] -> [B Ho Wo, KH KW Cin], zeros outside the image"""
    pb = max(0, (g.Ho - 1) * g.S + g.KH - g.H - g.PT)
    pr = max(0, (g.Wo - 1) * g.S + g.KW - g.W - g.PL)
    xp = np.pad(np.asarray(x, dtype), ((0, 0), (g.PT, pb), (g.PL, pr), (0, 0)))
    cols = np.empty((g.B, g.Ho, g.Wo, g.KH, g.KW, x.shape[-1]), dtype)
    for i in range(g.KH):
        for j in range(g.KW):
            cols[:, :, :, i, j] = xp[:, i:i + (g.Ho - 1) * g.S + 1:g.S, j:j + (g.Wo - 1) * g.S + 1:g.S]
    return cols.reshape(g.B * g.Ho * g.Wo, -1)


def conv_wgrad(x, dz, g, stem=False, dtype=np.float64):
    """x [B, H, W, Cin], dz [B, Ho, Wo, Cout] (undilated, logical values: x3 callers pass hi + lo) -> dw in the device layout:
    [Cout][Kpad] (stem: [K][Cout]), zero padding columns.  dtype float32: the restatement (a numpy float32 matmul)"""
    cols = im2col(x, g, dtype)
    d = np.asarray(dz, dtype).reshape(-1, g.Cout)
    K = cols.shape[1]
    if stem:
        return cols.T @ d
    out = np.zeros((g.Cout, kpad(K)), dtype)
    out[:, :K] = d.T @ cols
    return out


def conv_dgrad(dz, w, g, dtype=np.float64):
    """dz [B, Ho, Wo, Cout] (undilated values), w [Cout][>= K] the filter values the device multiplies by -> the contribution
    to gx [B, H, W, Cin]"""
    K = g.KH * g.KW * g.Cin
    d = np.asarray(dz, dtype).reshape(-1, g.Cout)
    dcols = (d @ np.asarray(w, dtype)[:, :K]).reshape(g.B, g.Ho, g.Wo, g.KH, g.KW, g.Cin)
    Hp = max(g.H + g.PT, (g.Ho - 1) * g.S + g.KH)
    Wp = max(g.W + g.PL, (g.Wo - 1) * g.S + g.KW)
    gx = np.zeros((g.B, Hp, Wp, g.Cin), dtype)
    for i in range(g.KH):
        for j in range(g.KW):
            gx[:, i:i + (g.Ho - 1) * g.S + 1:g.S, j:j + (g.Wo - 1) * g.S + 1:g.S] += dcols[:, :, :, i, j]
    return gx[:, g.PT:g.PT + g.H, g.PL:g.PL + g.W]


def pack_bwd(w_master, g, dtype):
    """master [Cout][Kpad] -> the backward-data filter [Cin][Kpad2] (float32 values, bit-exact): k2 = tap2 Cout + co with the
    flipped tap tap2 = (KH-1-kh) KW + (KW-1-kw); 'bf16': RNE; 'x3': k2 = tap2 3 Cout + region Cout + co with the regions
    [W_hi | W_hi | W_lo]; zero padding"""
    K = g.KH * g.KW * g.Cin
    w = np.asarray(w_master, np.float32)[:, :K].reshape(g.Cout, g.KH, g.KW, g.Cin)
    t = np.ascontiguousarray(w[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))        # [Cin][KH][KW][Cout], taps flipped
    if dtype == 'x3':
        hi, lo = split3(t)
        t = np.concatenate([hi, hi, lo], -1)
    elif dtype == 'bf16':
        t = bf16_round(t)
    t = t.reshape(g.Cin, -1)
    out = np.zeros((g.Cin, kpad(t.shape[1])), np.float32)
    out[:, :t.shape[1]] = t
    return out


def unpack_bwd(wb, g, dtype):
    """the filter VALUES a packed backward-data filter stands for, as [Cout][K] (x3: W_hi + W_lo), float64"""
    r = 3 if dtype == 'x3' else 1
    t = np.asarray(wb, np.float64)[:, :g.KH * g.KW * r * g.Cout].reshape(g.Cin, g.KH, g.KW, r, g.Cout)
    t = t[:, :, :, 0] + t[:, :, :, 2] if r == 3 else t[:, :, :, 0]
    return np.ascontiguousarray(t[:, ::-1, ::-1, :].transpose(3, 1, 2, 0)).reshape(g.Cout, -1)


def max_pool_grad(x, dy, g, dtype=np.float64):
    """x [B, H, W, C], dy [B, Ho, Wo, C] -> the contribution to dx.  Every window gives its dy to its FIRST maximum in
    (kh, kw) scan order (strict >; taps outside the image are -inf); a pixel's windows are added in (ho, wo) order, so dtype
    float32 restates the kernels' sums bit for bit"""
    x = np.asarray(x, np.float64)
    dy = np.asarray(dy, dtype)
    dx = np.zeros((g.B, g.H, g.W, x.shape[-1]), dtype)
    bi, ci = np.meshgrid(np.arange(g.B), np.arange(x.shape[-1]), indexing='ij')
    for ho in range(g.Ho):
        for wo in range(g.Wo):
            best = np.full((g.B, x.shape[-1]), -np.inf)
            ah = np.full(best.shape, -1)
            aw = np.full(best.shape, -1)
            for kh in range(g.KH):
                h2 = ho * g.S - g.PT + kh
                if not 0 <= h2 < g.H:
                    continue
                for kw in range(g.KW):
                    w2 = wo * g.S - g.PL + kw
                    if not 0 <= w2 < g.W:
                        continue
                    v = x[:, h2, w2]
                    m = v > best
                    best = np.where(m, v, best)
                    ah = np.where(m, h2, ah)
                    aw = np.where(m, w2, aw)
            ok = ah >= 0
            np.add.at(dx, (bi[ok], ah[ok], aw[ok], ci[ok]), dy[:, ho, wo][ok])
    return dx


def _valid_taps(g):
    ones = np.zeros((g.H + g.PT + g.KH + g.S * g.Ho, g.W + g.PL + g.KW + g.S * g.Wo))
    ones[g.PT:g.PT + g.H, g.PL:g.PL + g.W] = 1
    cnt = np.zeros((g.Ho, g.Wo))
    for i in range(g.KH):
        for j in range(g.KW):
            cnt += ones[i:i + (g.Ho - 1) * g.S + 1:g.S, j:j + (g.Wo - 1) * g.S + 1:g.S]
    return cnt


def avg_pool_grad(dy, g, dtype=np.float64, mean=False):
    """dy [B, Ho, Wo, C] -> the contribution to dx: every window spreads dy / (its taps inside the image) (mean: / KH KW, the
    VALID window of the head pool) over the pixels it covers"""
    dy = np.asarray(dy, dtype)
    cnt = np.full((g.Ho, g.Wo), float(g.KH * g.KW)) if mean else _valid_taps(g)
    gv = dy * (dtype(1) / cnt.astype(dtype))[None, :, :, None] if dtype == np.float32 else dy / cnt[None, :, :, None]
    Hp = max(g.H + g.PT, (g.Ho - 1) * g.S + g.KH)
    Wp = max(g.W + g.PL, (g.Wo - 1) * g.S + g.KW)
    dx = np.zeros((g.B, Hp, Wp, dy.shape[-1]), dtype)
    for ho in range(g.Ho):                  # (ho, wo) order per pixel, as the gather kernel adds
        for wo in range(g.Wo):
            dx[:, ho * g.S:ho * g.S + g.KH, wo * g.S:wo * g.S + g.KW] += gv[:, ho:ho + 1, wo:wo + 1]
    return dx[:, g.PT:g.PT + g.H, g.PL:g.PL + g.W]


def mean_pool_grad(dy, g, dtype=np.float64):
    return avg_pool_grad(dy, g, dtype, mean=True)


# ----------------------------------------------------------------------------------------------- figures -------------
def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))


def elementwise_excess(got, ref, tol):
    """largest |a - b| / (tol |b| + tol rms(b)) (gpu_util.elementwise_excess, restated so that this file needs numpy alone)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (tol * np.abs(ref) + tol * (np.sqrt(np.mean(ref * ref)) + 1e-30))).max())


# ----------------------------------------------------------------------------------------------- case tables ---------
# activation gradient: name -> (B, Ho, Wo, C, yc (logical channels of the output buffer), dst_coff, S)
ACT_CASES = {
    'c40_small': (1, 5, 7, 40, 40, 0, 1),                 # P = 35: below one 64-pixel block; C / EPC ragged in the 64-channel group
    'c40_slice_ragged': (3, 9, 7, 40, 72, 24, 1),         # P = 189: three blocks, the last of 61 pixels; a slice of a wider buffer
    'c192_blocks': (2, 17, 17, 192, 192, 0, 1),           # P = 578, three channel groups
    'c192_slice_s2': (2, 8, 8, 192, 224, 32, 2),          # zero-dilated into 15 x 15
    'c40_s2': (3, 4, 5, 40, 40, 0, 2)}

# weight gradient: the pixel counts every kernel form runs at: name -> (B, H, W)
PIXELS = {'p189': (3, 9, 7),        # one split, 29-pixel tail of the last 32-pixel step
          'p578': (2, 17, 17)}      # three splits 224 / 224 / 130; the batch boundary (pixel 289) inside a 32-pixel step
# conv_wgrad_tr_kernel<BM, BN> (bf16 and x3 plans): name -> (Cin, Cout, k)
TR_FORMS = {
    'tr64x64': (32, 48, (3, 3)),            # K = 288: ragged last k tile, ragged Cout tile
    'tr64x128': (96, 64, (3, 3)),           # K = 864, Kpad = 896
    'tr128x64': (32, 128, (3, 3)),
    'tr128x128': (128, 128, (1, 3)),
    'tr128x128_c384': (128, 384, (1, 3))}
# geometries (on the 64 x 64 form and the fp32 kernel): name -> (B, H, W, Cin, Cout, k, S, pad, xc, src_coff)
GEOMETRIES = {
    '1x1': (2, 17, 17, 32, 48, (1, 1), 1, 'SAME', 32, 0),
    '1x7': (2, 17, 17, 32, 48, (1, 7), 1, 'SAME', 32, 0),
    '7x1': (2, 17, 17, 32, 48, (7, 1), 1, 'SAME', 32, 0),
    '5x5': (3, 9, 7, 32, 48, (5, 5), 1, 'SAME', 32, 0),
    '3x3s2_odd': (2, 17, 17, 32, 48, (3, 3), 2, 'VALID', 32, 0),
    '3x3s2_even': (2, 16, 18, 32, 48, (3, 3), 2, 'VALID', 32, 0),
    '3x3_src_slice': (3, 9, 7, 32, 48, (3, 3), 1, 'SAME', 80, 32)}
# conv_wgrad_kernel<float, false>: name -> (Cin, Cout, k); Cin 12: the backward-data conv needs Cin % 16 == 0, so the source
# has no gradient buffer and only the weight gradient runs
F32_FORMS = {'f32_c12': (12, 48, (3, 3)), 'f32_c32': (32, 48, (3, 3))}
STEM_IMAGES = (35, 34)              # 3 x 3 / 2 VALID, Cin 3 -> Cout 32, B 2

# backward-data over the kernel ids: name -> (B, H, W, Cin, Cout, k, S, pad)
DGRAD_CASES = {'3x3_64_64': (2, 17, 17, 64, 64, (3, 3), 1, 'SAME'), '3x3s2_96_32': (2, 17, 17, 96, 32, (3, 3), 2, 'VALID')}

# fused activation gradient: p (1x1 or 3x3, Cin 32 -> C) feeds c (3x3 SAME, C -> 64) on 17 x 17 maps, B 3
FUSED_C = (48, 128)

# pools: name -> (kind, B, H, W, C, k, S, pad)
POOL_CASES = {
    'max_s2_16_valid_c40': (2, 2, 16, 16, 40, 3, 2, 'VALID'),
    'max_s2_16_pad_c64': (2, 2, 16, 16, 64, 3, 2, (1, 1)),
    'max_s2_17_valid_c64': (2, 2, 17, 17, 64, 3, 2, 'VALID'),
    'max_s2_17_pad_c40': (2, 2, 17, 17, 40, 3, 2, (1, 1)),
    'max_s2_35x33_valid_c40': (2, 1, 35, 33, 40, 3, 2, 'VALID'),
    'max_s2_35x33_pad_c64': (2, 1, 35, 33, 64, 3, 2, (1, 1)),
    'max_s1_same': (2, 2, 13, 11, 40, 3, 1, 'SAME'),
    'avg_5x5': (3, 3, 5, 5, 40, 3, 1, 'SAME'),
    'avg_13x11': (3, 2, 13, 11, 64, 3, 1, 'SAME'),
    'mean_5x5': (4, 3, 5, 5, 64, 5, 1, 'VALID'),
    'mean_8x8_on_9x9': (4, 2, 9, 9, 40, 8, 1, 'VALID')}


def seed_of(name):
    """a case's seed from its name (stable across processes, unlike hash())"""
    s = 0
    for ch in name:
        s = (s * 131 + ord(ch)) % 1000003
    return s


def conv_cases():
    """every single-conv case of the GPU suite: name -> dict(plan, g, xc, src_coff, stem, dgrad)"""
    out = {}
    for plan in ('bf16', 'x3'):
        for fn, (cin, cout, k) in TR_FORMS.items():
            for pn, (B, H, W) in PIXELS.items():
                out['%s-%s-%s' % (plan, fn, pn)] = dict(plan=plan, g=geo(B, H, W, cin, cout, k, 1, 'SAME'), xc=cin, src_coff=0,
                                                       stem=False, dgrad=True)
    for plan in PLANS:
        for gn, (B, H, W, cin, cout, k, s, pad, xc, sc) in GEOMETRIES.items():
            out['%s-%s' % (plan, gn)] = dict(plan=plan, g=geo(B, H, W, cin, cout, k, s, pad), xc=xc, src_coff=sc, stem=False,
                                             dgrad=True)
    for fn, (cin, cout, k) in F32_FORMS.items():
        for pn, (B, H, W) in PIXELS.items():
            out['f32-%s-%s' % (fn, pn)] = dict(plan='f32', g=geo(B, H, W, cin, cout, k, 1, 'SAME'), xc=cin, src_coff=0,
                                               stem=False, dgrad=cin % 16 == 0)
    for plan in PLANS:
        for n in STEM_IMAGES:
            out['%s-stem-%d' % (plan, n)] = dict(plan=plan, g=geo(2, n, n, 3, 32, 3, 2, 'VALID'), xc=3, src_coff=0, stem=True,
                                                 dgrad=False)
    return out


def conv_operands(name, case):
    """the operands of one conv case: logical float32 x [B, H, W, xc], y and dy [B, Ho, Wo, Cout], scale, master"""
    g, plan, s = case['g'], case['plan'], seed_of(name)
    if case['stem']:
        x = _rng(s, 3).uniform(-1, 1, (g.B, g.H, g.W, 3)).astype(np.float32)        # the fp32 image of every plan
    else:
        x = make_x(s, (g.B, g.H, g.W, case['xc']), plan)
    return dict(x=x, y=make_y(s, (g.B, g.Ho, g.Wo, g.Cout), plan), dy=make_dy(s, (g.B, g.Ho, g.Wo, g.Cout), plan),
                scale=make_scale(s, g.Cout), w=make_master(s, g))


def conv_reference(case, ops, dtype=np.float64):
    """-> dict(dz (stored values, device layout), dbeta, dw, wb (packed filter), gx (contribution to the source slice)) of
    one conv case; dtype float32: the restatement of dw / gx"""
    g, plan = case['g'], case['plan']
    dz, dbeta = act_grad(ops['y'], ops['dy'], ops['scale'], plan, g.S)
    dzv = logical(dz[:, ::g.S, ::g.S], plan, dtype)                 # the stored d conv, undilated
    xs = ops['x'][..., case['src_coff']:case['src_coff'] + g.Cin]
    if case['stem'] and plan == 'bf16':
        xs = bf16_round(xs)                                         # the kernel rounds the image on its way into the LDS
    elif case['stem'] and plan == 'x3':
        xs = representable(xs, 'x3')                                # parts 0 / 2: bf16(x), part 1: bf16(x - bf16(x))
    out = dict(dz=dz, dbeta=dbeta, dw=conv_wgrad(xs, dzv, g, case['stem'], dtype))
    if case['dgrad']:
        out['wb'] = pack_bwd(ops['w'], g, plan)
        out['gx'] = conv_dgrad(dzv, unpack_bwd(out['wb'], g, plan), g, dtype)
    return out


def conv_bars(case):
    """(dw bar, gx bar, gx is a bf16 store)"""
    plan = case['plan']
    return (X3_BAR if plan == 'x3' else F32_BAR, {'f32': F32_BAR, 'bf16': BF16_STORE_BAR, 'x3': X3_BAR}[plan], plan == 'bf16')


def dgrad_case(name, plan):
    B, H, W, cin, cout, k, s, pad = DGRAD_CASES[name]
    return dict(plan=plan, g=geo(B, H, W, cin, cout, k, s, pad), xc=cin, src_coff=0, stem=False, dgrad=True)


def fused_operands(Cc, plan, p_stride=1):
    """the two-conv chain p -> c of the fused activation gradient: p 1x1 (p_stride 2: 3x3 / 2 VALID from 35 x 35, which must not
    fuse) 32 -> Cc, c 3x3 SAME Cc -> 64, on 17 x 17 maps, B 3.  The reader's d conv and filter are small dyadic numbers -- dy_c in
    eighths (mean 1), scale_c 1/2, 1 or 2, w_c in quarters -- so the fp32 accumulators of its backward-data launch are exact
    whatever the summation order, and what the fused epilogue makes of them can be compared bit for bit"""
    s = seed_of('fused%d' % Cc)
    gp = geo(3, 17, 17, 32, Cc, (1, 1), 1, 'SAME') if p_stride == 1 else geo(3, 35, 35, 32, Cc, (3, 3), 2, 'VALID')
    gc = geo(3, 17, 17, Cc, 64, (3, 3), 1, 'SAME')
    r = _rng(s, 8)
    w_c = np.zeros((64, kpad(9 * Cc)), np.float32)
    w_c[:, :9 * Cc] = r.integers(-7, 8, (64, 9 * Cc)) / 4.0
    return dict(gp=gp, gc=gc, x_p=make_x(s, (gp.B, gp.H, gp.W, 32), plan), y_p=make_y(s + 1, (3, 17, 17, Cc), plan),
                scale_p=make_scale(s, Cc), w_p=make_master(s, gp), y_c=make_y(s + 2, (3, 17, 17, 64), plan),
                dy_c=(r.integers(1, 16, (3, 17, 17, 64)) / 8.0).astype(np.float32),
                scale_c=np.array([0.5, 1.0, 2.0], np.float32)[r.integers(0, 3, 64)], w_c=w_c)


def pool_geo(case):
    kind, B, H, W, C, k, S, pad = case
    return geo(B, H, W, C, C, k, S, pad)


def pool_operands(name, case, plan, ties=False):
    """x (logical float32; x3: split3 gives the regions), dy (bf16 plan: bf16 values; kind 4: fp32 in every plan)"""
    kind = case[0]
    g, s = pool_geo(case), seed_of(name)
    if ties:
        x = tie_map(s, (g.B, g.H, g.W, g.Cin))
    else:
        x = make_x(s, (g.B, g.H, g.W, g.Cin), plan)
    dy = make_dy(s, (g.B, g.Ho, g.Wo, g.Cin), 'f32' if kind == 4 else plan)
    return x, dy


def pool_reference(case, x, dy, dtype=np.float64):
    g = pool_geo(case)
    if case[0] == 2:
        return max_pool_grad(x, dy, g, dtype)
    return avg_pool_grad(dy, g, dtype) if case[0] == 3 else mean_pool_grad(dy, g, dtype)
