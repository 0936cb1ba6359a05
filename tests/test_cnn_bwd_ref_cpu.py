"""What the op tests of the CNN backward kernels (tests/test_gpu_cnn_bwd_ops.py) rest on, checked without a GPU, on the
builders, shapes and seeds of every GPU case: the float64 references of tests/cnn_bwd_ref.py agree with the oracle's own
backward primitives (oracle/cnn_ref.py: an independent float32 implementation, arg-max ties included) and with central
differences of a float64 forward; the bit-exact references have the bits they claim; and the float32 restatement of each
reference stays inside a quarter of its op's bar, so regimes.bar() returns that bar unchanged and three quarters of it are the
kernel's."""
import numpy as np
import pytest

from oracle import cnn_ref
from tests import cnn_bwd_ref as R
from tests import regimes

ORACLE_TOL = 1e-5
CONV_CASES = R.conv_cases()


def _hwio(w, g):
    return np.ascontiguousarray(w[:, :g.KH * g.KW * g.Cin].reshape(g.Cout, g.KH, g.KW, g.Cin).transpose(1, 2, 3, 0))


def _padded(x, g, value=0.0):
    """x with the geometry's padding made explicit, so that the oracle's VALID form of the op has the same windows"""
    pb = max(0, (g.Ho - 1) * g.S + g.KH - g.H - g.PT)
    pr = max(0, (g.Wo - 1) * g.S + g.KW - g.W - g.PL)
    xp = np.pad(x, ((0, 0), (g.PT, pb), (g.PL, pr), (0, 0)), constant_values=value)
    assert cnn_ref.out_size(xp.shape[1], g.KH, g.S, 'VALID')[0] == g.Ho and cnn_ref.out_size(xp.shape[2], g.KW, g.S, 'VALID')[0] == g.Wo
    return xp


def _crop(dxp, g):
    return dxp[:, g.PT:g.PT + g.H, g.PL:g.PL + g.W]


def test_case_tables_reach_the_paths_they_name():
    """the launcher's own arithmetic (launch_wgrad_tr of csrc/conv_bwd.hip) on the shapes of the tables: tile form, pixel splits,
    the ragged tail"""
    def form(g):
        K = g.KH * g.KW * g.Cin
        return (128 if g.Cout % 128 == 0 else 64, 128 if R.kpad(K) % 128 == 0 and K >= 256 else 64)
    want = {'tr64x64': (64, 64), 'tr64x128': (64, 128), 'tr128x64': (128, 64), 'tr128x128': (128, 128), 'tr128x128_c384': (128, 128)}
    for fn, bmbn in want.items():
        for pn in R.PIXELS:
            for plan, parts in (('bf16', 1), ('x3', 3)):
                g = CONV_CASES['%s-%s-%s' % (plan, fn, pn)]['g']
                assert form(g) == bmbn, (fn, form(g))
                K, P = g.KH * g.KW * g.Cin, g.B * g.Ho * g.Wo
                tiles = -(-K // bmbn[1]) * -(-g.Cout // bmbn[0]) * parts
                S = max(1, min(1024 // tiles, -(-P // 256)))
                per = -(-(-(-P // S)) // 32) * 32
                splits = [min(per, P - s * per) for s in range(-(-P // per))]
                assert splits == ([189] if pn == 'p189' else [224, 224, 130]), (fn, pn, plan, splits)
    assert 189 % 32 == 29 and 289 % 32 != 0          # the 29-pixel tail; the batch boundary inside a 32-pixel step
    g = CONV_CASES['bf16-tr64x64-p189']['g']
    assert g.KH * g.KW * g.Cin == 288 and g.Cout % 64 == 48          # ragged last k tile, ragged Cout tile
    g = CONV_CASES['bf16-tr64x128-p189']['g']
    assert (g.KH * g.KW * g.Cin, R.kpad(g.KH * g.KW * g.Cin)) == (864, 896)
    assert CONV_CASES['f32-f32_c12-p189']['g'].Cin * 9 == 108 and not CONV_CASES['f32-f32_c12-p189']['dgrad']
    for name, (B, Ho, Wo, Cc, yc, coff, S) in R.ACT_CASES.items():
        assert Cc % 8 == 0 and coff % 8 == 0 and coff + Cc <= yc
    assert (40 // 8) % 8 != 0 and 35 < 64 and 189 % 64 == 61


@pytest.mark.parametrize('name', sorted(CONV_CASES))
def test_conv_references_agree_with_the_oracle_and_the_float32_restatement_is_small(name):
    case = CONV_CASES[name]
    g, plan = case['g'], case['plan']
    ops = R.conv_operands(name, case)
    ref = R.conv_reference(case, ops)
    r32 = R.conv_reference(case, ops, np.float32)
    # the stored d conv: the plan's bits, zeros between dilated pixels, and the value 1[y > 0] dy scale
    dz = ref['dz']
    if plan != 'f32':
        assert not (R.bits(dz) & 0xFFFF).any()
    if plan == 'x3':
        C_ = g.Cout
        np.testing.assert_array_equal(R.bits(dz[..., :C_]), R.bits(dz[..., 2 * C_:]))
    if g.S == 2:
        assert dz.shape[1:3] == ((g.Ho - 1) * 2 + 1, (g.Wo - 1) * 2 + 1)
        assert not dz[:, 1::2].any() and not dz[:, :, 1::2].any()
    dzv = R.logical(dz[:, ::g.S, ::g.S], plan)
    want = np.where(ops['y'] > 0, ops['dy'].astype(np.float64), 0) * ops['scale'].astype(np.float64)
    assert R.rel_err(dzv, want) <= {'f32': 2.0 ** -23, 'bf16': 2.0 ** -8, 'x3': 2.0 ** -15}[plan]
    assert R.rel_err(ref['dbeta'], np.where(ops['y'] > 0, ops['dy'], 0).sum((0, 1, 2), dtype=np.float64)) == 0
    frac = float((ops['y'] <= 0).mean())
    assert 0.4 < frac < 0.6, frac
    # the oracle's conv2d_bwd on the same stored operands
    xs = ops['x'][..., case['src_coff']:case['src_coff'] + g.Cin]
    if case['stem']:
        xs = R.representable(xs, plan)
    w_used = R.unpack_bwd(ref['wb'], g, plan) if case['dgrad'] else ops['w'][:, :g.KH * g.KW * g.Cin]
    dxp, dw = cnn_ref.conv2d_bwd(_padded(xs, g), _hwio(np.asarray(w_used, np.float32), g), dzv.astype(np.float32), g.S, 'VALID')
    dw_dev = dw.reshape(-1, g.Cout) if case['stem'] else dw.reshape(-1, g.Cout).T
    K = g.KH * g.KW * g.Cin
    got_dw = ref['dw'] if case['stem'] else ref['dw'][:, :K]
    e_dw = R.rel_err(got_dw, dw_dev)
    assert e_dw <= ORACLE_TOL, e_dw
    if not case['stem']:
        assert not ref['dw'][:, K:].any()
    dw_bar, gx_bar, _ = R.conv_bars(case)
    r_dw = R.rel_err(r32['dw'], ref['dw'])
    assert r_dw <= dw_bar / 4 and regimes.bar(dw_bar, r_dw) == dw_bar, r_dw
    assert R.elementwise_excess(r32['dw'], ref['dw'], dw_bar) <= 0.25
    if case['dgrad']:
        e_gx = R.rel_err(ref['gx'], _crop(dxp, g))
        assert e_gx <= ORACLE_TOL, e_gx
        r_gx = R.rel_err(r32['gx'], ref['gx'])
        assert r_gx <= gx_bar / 4 and regimes.bar(gx_bar, r_gx) == gx_bar, r_gx
        # the packed filter: flipped taps, the plan's bits, zero padding, and the values of the master
        wb = ref['wb']
        r = 3 if plan == 'x3' else 1
        assert wb.shape == (g.Cin, R.kpad(g.KH * g.KW * r * g.Cout)) and not wb[:, g.KH * g.KW * r * g.Cout:].any()
        if plan != 'f32':
            assert not (R.bits(wb) & 0xFFFF).any()
        assert R.rel_err(w_used, ops['w'][:, :K]) <= {'f32': 0, 'bf16': 2.0 ** -8, 'x3': 2.0 ** -15}[plan]


def test_pack_bwd_element_by_element():
    """the index formula of pack_bwd_weights_kernel / pack_bwd_x3_value, restated with plain loops on one small filter"""
    g = R.geo(1, 5, 5, 8, 16, (3, 2), 1, 'SAME')
    w = R.make_master(7, g)
    Kp = w.shape[1]
    for plan in R.PLANS:
        wb = R.pack_bwd(w, g, plan)
        r = 3 if plan == 'x3' else 1
        for ci in range(g.Cin):
            for k2 in range(wb.shape[1]):
                if k2 >= g.KH * g.KW * r * g.Cout:
                    want = np.float32(0)
                else:
                    tap2, rr = divmod(k2, r * g.Cout)
                    region, co = divmod(rr, g.Cout)
                    kh, kw = g.KH - 1 - tap2 // g.KW, g.KW - 1 - tap2 % g.KW
                    v = w.reshape(-1)[co * Kp + (kh * g.KW + kw) * g.Cin + ci]
                    hi = R.bf16_round(np.float32(v))
                    want = v if plan == 'f32' else hi if region < 2 else R.bf16_round(np.float32(v - hi))
                assert R.bits(wb[ci, k2]) == R.bits(np.float32(want)), (plan, ci, k2)


@pytest.mark.parametrize('plan', R.PLANS)
@pytest.mark.parametrize('name', sorted(R.ACT_CASES))
def test_act_grad_reference(name, plan):
    B, Ho, Wo, Cc, yc, coff, S = R.ACT_CASES[name]
    s = R.seed_of(name)
    y, dy, sc = R.make_y(s, (B, Ho, Wo, Cc), plan), R.make_dy(s, (B, Ho, Wo, Cc), plan), R.make_scale(s, Cc)
    flat = y.reshape(-1)
    assert flat[0] == 0 and not np.signbit(flat[0]) and flat[1] == 0 and np.signbit(flat[1]) and flat[2] == R.BF16_MIN_NORMAL
    np.testing.assert_array_equal(R.bits(R.representable(y, plan)), R.bits(y))
    np.testing.assert_array_equal(R.logical(R.store(y, plan), plan, np.float32), y)       # the stored regions sum back to y
    assert abs(float(dy.mean()) - 1) < 0.1
    dz, dbeta = R.act_grad(y, dy, sc, plan, S)
    assert dz.shape == (B, (Ho - 1) * S + 1, (Wo - 1) * S + 1, Cc * (3 if plan == 'x3' else 1))
    z = dz[:, ::S, ::S]
    assert not R.bits(z[0, 0, 0, :2]).any() and z[0, 0, 0, 2] == R.store(np.float32(dy[0, 0, 0, 2] * sc[2]), plan).reshape(-1)[0]
    # masked elements are +0.0 (the kernel multiplies a selected +0.0 by a positive scale)
    assert not R.bits(R.logical(z, plan, np.float32))[y <= 0].any()
    r32 = np.where(y > 0, dy, np.float32(0)).sum((0, 1, 2), dtype=np.float32)
    e = R.rel_err(r32, dbeta)
    assert e <= R.F32_BAR / 4 and regimes.bar(R.F32_BAR, e) == R.F32_BAR, e


def _windows(xp, g):
    return np.stack([xp[:, i:i + (g.Ho - 1) * g.S + 1:g.S, j:j + (g.Wo - 1) * g.S + 1:g.S] for i in range(g.KH) for j in range(g.KW)])


POOL_PARAMS = [(n, p, t) for n in sorted(R.POOL_CASES) for p in R.PLANS for t in ((False, True) if R.POOL_CASES[n][0] == 2 else (False,))]


@pytest.mark.parametrize('name,plan,ties', POOL_PARAMS)
def test_pool_references_agree_with_the_oracle(name, plan, ties):
    case = R.POOL_CASES[name]
    kind, g = case[0], R.pool_geo(case)
    x, dy = R.pool_operands(name, case, plan, ties)
    ref = R.pool_reference(case, x, dy)
    r32 = R.pool_reference(case, x, dy, np.float32)
    assert r32.dtype == np.float32
    if kind == 2:
        xp = _padded(x, g, -np.inf)
        # the same pixels receive a gradient (the arg-maxima agree, ties included); sums of at most four dy, which the oracle
        # adds in float32 in tap order
        want = _crop(cnn_ref.max_pool_bwd(xp, dy, g.KH, g.S, 'VALID'), g)
        np.testing.assert_array_equal(ref != 0, want != 0)
        np.testing.assert_allclose(ref, want, rtol=1e-6, atol=0)
        assert R.rel_err(ref, want) <= ORACLE_TOL
        win = _windows(xp, g)
        tied = float(((win == win.max(0)).sum(0) > 1).mean())
        print('%s %s: %.0f %% of the windows have tied maxima' % (name, plan, 100 * tied))
        assert (tied > 0.5) if ties else (tied < 0.05), tied
    elif kind == 3:
        assert R.rel_err(ref, cnn_ref.avg_pool_bwd(x.shape, dy, g.KH, g.S, 'SAME')) <= ORACLE_TOL
    else:
        assert R.rel_err(ref, cnn_ref.avg_pool_bwd(x.shape, dy, (g.KH, g.KW), g.S, 'VALID')) <= ORACLE_TOL
    e = R.rel_err(r32, ref)
    assert e <= R.F32_BAR / 4 and regimes.bar(R.F32_BAR, e) == R.F32_BAR, e
    assert R.elementwise_excess(r32, ref, R.F32_BAR) <= 0.25
    if kind != 4 or (g.Ho - 1) * g.S + g.KH == g.H:          # every window passes its whole gradient on
        assert abs(float(ref.sum()) / float(np.asarray(dy, np.float64).sum()) - 1) < 1e-9


def test_max_pool_first_maximum_by_hand():
    """one 3 x 3 window over constant input: the whole gradient lands on the first tap; with padding, on the first tap INSIDE the
    image"""
    x = np.ones((1, 3, 3, 1), np.float32)
    dy = np.full((1, 1, 1, 1), 5.0, np.float32)
    dx = R.max_pool_grad(x, dy, R.geo(1, 3, 3, 1, 1, 3, 2, 'VALID'))
    assert dx[0, 0, 0, 0] == 5 and dx.sum() == 5
    g = R.geo(1, 3, 3, 1, 1, 3, 2, (1, 1))              # windows at rows / columns -1..1 and 1..3
    dx = R.max_pool_grad(x, np.arange(1, 5, dtype=np.float32).reshape(1, 2, 2, 1), g)
    np.testing.assert_array_equal(dx[0, :, :, 0], [[1, 2, 0], [3, 4, 0], [0, 0, 0]])
    x[0, 1, 1, 0] = 2                                   # a strict maximum inside all four windows
    dx = R.max_pool_grad(x, np.arange(1, 5, dtype=np.float32).reshape(1, 2, 2, 1), g)
    assert dx[0, 1, 1, 0] == 10 and dx.sum() == 10


def test_central_differences_of_a_float64_forward():
    """one tiny conv (stride 2, padded, through ReLU and the BatchNorm scale) and one tiny max / avg pool: the references are
    the gradients of the forward they claim to differentiate"""
    rng = np.random.default_rng(3)
    g = R.geo(2, 5, 4, 3, 4, (3, 2), 2, (1, 1))
    x = rng.standard_normal((g.B, g.H, g.W, g.Cin))
    w = rng.standard_normal((g.Cout, g.KH * g.KW * g.Cin))
    scale, shift = rng.uniform(0.5, 1.5, g.Cout), rng.standard_normal(g.Cout)
    dy = 1 + 0.5 * rng.standard_normal((g.B, g.Ho, g.Wo, g.Cout))

    def fwd(x_, w_, beta_):
        z = (R.im2col(x_, g) @ w_.T).reshape(g.B, g.Ho, g.Wo, g.Cout) * scale + beta_
        return np.maximum(z, 0)

    y = fwd(x, w, shift)
    assert np.abs(y[y > 0]).min() > 1e-4               # no unit sits on the kink
    dzs, dbeta = np.where(y > 0, dy, 0) * scale, np.where(y > 0, dy, 0).sum((0, 1, 2))
    dw, gx = R.conv_wgrad(x, dzs, g)[:, :w.shape[1]], R.conv_dgrad(dzs, w, g)
    loss = lambda *a: float((fwd(*a) * dy).sum())
    h = 1e-6

    def num(arr, which):
        out = np.zeros_like(arr)
        for i in np.ndindex(arr.shape):
            a, b = arr.copy(), arr.copy()
            a[i] += h
            b[i] -= h
            args = [x, w, shift]
            args[which] = a
            lp = loss(*args)
            args[which] = b
            out[i] = (lp - loss(*args)) / (2 * h)
        return out
    assert R.rel_err(gx, num(x, 0)) < 1e-7
    assert R.rel_err(dw, num(w, 1)) < 1e-7
    assert R.rel_err(dbeta, num(shift, 2)) < 1e-7
    # the same dz through the float32 stores: the bit-exact act_grad is this value rounded once
    dz32, db32 = R.act_grad(y.astype(np.float32), dy.astype(np.float32), scale.astype(np.float32), 'f32', 2)
    assert R.rel_err(dz32[:, ::2, ::2], dzs) < 1e-6 and R.rel_err(db32, dbeta) < 1e-6
    # pools
    for kind, k, s, pad in ((2, 3, 2, (1, 1)), (3, 3, 1, 'SAME'), (4, 3, 1, 'VALID')):
        pg = R.geo(2, 5, 4, 3, 3, k, s, pad)
        px = rng.standard_normal((pg.B, pg.H, pg.W, 3))
        pdy = 1 + 0.5 * rng.standard_normal((pg.B, pg.Ho, pg.Wo, 3))

        def pfwd(x_):
            fill = -np.inf if kind == 2 else 0.0
            pb, pr = max(0, (pg.Ho - 1) * s + k - pg.H - pg.PT), max(0, (pg.Wo - 1) * s + k - pg.W - pg.PL)
            xp = np.pad(x_, ((0, 0), (pg.PT, pb), (pg.PL, pr), (0, 0)), constant_values=fill)
            win = np.stack([xp[:, i:i + (pg.Ho - 1) * s + 1:s, j:j + (pg.Wo - 1) * s + 1:s] for i in range(k) for j in range(k)])
            if kind == 2:
                return win.max(0)
            return win.sum(0) / (R._valid_taps(pg)[None, :, :, None] if kind == 3 else k * k)
        got = R.pool_reference((kind, pg.B, pg.H, pg.W, 3, k, s, pad), px, pdy)
        want = np.zeros_like(px)
        for i in np.ndindex(px.shape):
            a, b = px.copy(), px.copy()
            a[i] += h
            b[i] -= h
            want[i] = float(((pfwd(a) - pfwd(b)) * pdy).sum()) / (2 * h)
        assert R.rel_err(got, want) < 1e-7, kind


@pytest.mark.parametrize('Cc', R.FUSED_C)
def test_fused_chain_operands_make_the_accumulators_exact(Cc):
    """the fused activation gradient is compared bit for bit, so the backward-data accumulators it masks must not depend on a
    kernel's summation order: d conv of the reader and its filter are small dyadic numbers whose products and partial sums are
    exact in float32 (and in bf16 storage), whatever the order"""
    ops = R.fused_operands(Cc, 'bf16')
    gc = ops['gc']
    dz_c, _ = R.act_grad(ops['y_c'], ops['dy_c'], ops['scale_c'], 'bf16')
    np.testing.assert_array_equal(R.bits(dz_c), R.bits(R.act_grad(ops['y_c'], ops['dy_c'], ops['scale_c'], 'f32')[0]))
    np.testing.assert_array_equal(R.bits(R.bf16_round(ops['w_c'])), R.bits(ops['w_c']))
    g64 = R.conv_dgrad(dz_c, ops['w_c'], gc)
    g32 = R.conv_dgrad(dz_c, ops['w_c'], gc, np.float32)
    np.testing.assert_array_equal(g64, g32.astype(np.float64))
    # worst case of any partial sum: every product at its largest, all of one sign
    worst = np.abs(dz_c).max() * np.abs(ops['w_c']).max() * gc.KH * gc.KW * gc.Cout
    quantum = 2.0 ** -6              # dz_c in multiples of 1/16 (dy k/8 times a scale of 1/2, 1 or 2), the filter of 1/4
    assert worst / quantum < 2 ** 24 and not np.mod(g64 / quantum, 1).any()
    assert abs(float(ops['dy_c'].mean()) - 1) < 0.1
    dz_p, dbeta_p = R.fused_act_grad(g32, ops['y_p'], ops['scale_p'], 'bf16')
    unfused, _ = R.act_grad(ops['y_p'], R.bf16_round(g32), ops['scale_p'], 'bf16')
    assert (R.bits(dz_p) != R.bits(unfused)).any()          # the rounding of the intermediate gradient the fused form skips
    r32 = np.where(ops['y_p'] > 0, g32, np.float32(0)).sum((0, 1, 2), dtype=np.float32)
    assert R.rel_err(r32, dbeta_p) <= R.F32_BAR / 4
    # the two weight gradients of the chain at their bars
    for x_, dz_, g_ in ((ops['x_p'], dz_p, ops['gp']), (ops['y_p'], dz_c, gc)):
        ref, r = R.conv_wgrad(x_, dz_, g_), R.conv_wgrad(x_, dz_, g_, dtype=np.float32)
        e = R.rel_err(r, ref)
        assert e <= R.F32_BAR / 4 and regimes.bar(R.F32_BAR, e) == R.F32_BAR, e
        assert R.elementwise_excess(r, ref, R.F32_BAR) <= 0.25


@pytest.mark.parametrize('plan', R.PLANS)
@pytest.mark.parametrize('name', sorted(R.DGRAD_CASES))
def test_dgrad_cases_restatement(name, plan):
    case = R.dgrad_case(name, plan)
    ops = R.conv_operands(name, case)
    ref, r32 = R.conv_reference(case, ops), R.conv_reference(case, ops, np.float32)
    _, bar, _ = R.conv_bars(case)
    e = R.rel_err(r32['gx'], ref['gx'])
    assert e <= bar / 4 and regimes.bar(bar, e) == bar, e
    g = case['g']
    dxp, _ = cnn_ref.conv2d_bwd(_padded(ops['x'], g), _hwio(np.asarray(R.unpack_bwd(ref['wb'], g, plan), np.float32), g),
                                R.logical(ref['dz'][:, ::g.S, ::g.S], plan, np.float32), g.S, 'VALID')
    assert R.rel_err(ref['gx'], _crop(dxp, g)) <= ORACLE_TOL
