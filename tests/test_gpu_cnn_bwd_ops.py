"""The CNN backward (csrc/conv_bwd.hip) one launch at a time, each on operands the test builds, against float64 numpy
(tests/cnn_bwd_ref.py).  Only the public C ABI is used: comic_cnn_backward, comic_cnn_backward_sched,
comic_cnn_pack_bwd_filters and comic_cnn_backward_scratch_bytes on hand-built plans of one or two ops.  The backward reads
(x, y, dy, scale, w_master) and never runs a forward, so y is GIVEN: no ReLU mask or pool arg-max can differ between device and
reference, and each launch is held to the accuracy of its own arithmetic instead of the 1e-3 / 4e-2 per variable of the
whole-pass tests (tests/test_gpu_path.py).

Conventions (those of tests/test_gpu_exec_ops.py): what a launch writes is 0xFF before it; what it accumulates into (dw, d beta,
gx, dx) is prefilled with known non-zero values and everything outside its slice must come back untouched; every figure is
printed before it is asserted (pytest -s).  Bars: cnn_bwd_ref.F32_BAR / X3_BAR / BF16_STORE_BAR, each through regimes.bar() with
the float32 restatement of the reference on the same operands (tests/test_cnn_bwd_ref_cpu.py holds it below a quarter of the
bar); bit-exact claims with assert_array_equal on the bits."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import comic_amd._lib as L
from tests import cnn_bwd_ref as R
from tests import regimes
from tests.gpu_util import DEV, assert_close, elementwise_excess, lib, stream, sync

_TDT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'x3': torch.bfloat16}
_CODE = {'f32': 0, 'bf16': 1, 'x3': 1}
_ES = {'f32': 4, 'bf16': 2, 'x3': 2}
CONV_CASES = R.conv_cases()


# ------------------------------------------------------------------------------------------------- plumbing ----------
def act_dev(v, plan):
    """logical float32 values -> the activation buffer of the plan (x3: three bf16 regions)"""
    return torch.from_numpy(np.ascontiguousarray(R.store(v, plan))).to(_TDT[plan]).to(DEV)


def grad_dev(v, plan):
    """a gradient buffer: the plan's dtype; fp32 of the logical channels for x3"""
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(torch.bfloat16 if plan == 'bf16' else torch.float32).to(DEV)


def f32_dev(v):
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(DEV)


def host(t):
    return t.detach().float().cpu().numpy()


def wide(v, channels, coff, fill):
    """[..., C] placed at channel offset coff of a [..., channels] array, `fill` around it"""
    out = np.full(v.shape[:-1] + (channels,), fill, np.float32)
    out[..., coff:coff + v.shape[-1]] = v
    return out


def scratch_view(scratch, offset, shape, plan):
    """the d-conv tensor the device left at a byte offset of the scratch, as float32 values"""
    n = int(np.prod(shape))
    raw = scratch[offset:offset + n * _ES[plan]]
    return host(raw.view(_TDT[plan]).view(*shape))


def same_bits(got, want, what):
    np.testing.assert_array_equal(R.bits(got), R.bits(want), err_msg=what)
    print('  %-52s bit-exact (%d values)' % (what, np.asarray(got).size))


def chk(name, got, ref, op_bar, restated, elementwise=True):
    """max-norm (and element-wise) bound at regimes.bar(op_bar, restated); prints the figure first"""
    tol = regimes.bar(op_bar, restated)
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(got).all()
    e = R.rel_err(got, ref) if fin else float('nan')
    x = elementwise_excess(got, ref, tol) if (fin and elementwise) else float('nan')
    print('  %-52s err %.3e  element-wise %.2f  bar %.1e  [float32 restatement %.2e]' % (name, e, x, tol, restated))
    return assert_close(got, ref, tol, name, elementwise=elementwise)


def chk_bf16_store(name, got, prefill, ref, restated):
    """a bf16 read-modify-write store: bf16(prefill + result), the criterion test_conv_bn_relu uses for bf16 stores"""
    want = R.bf16_round((np.asarray(prefill, np.float64) + np.asarray(ref, np.float64)).astype(np.float32))
    return chk(name, got, want, R.BF16_STORE_BAR, restated, elementwise=False)


class Plan:
    """ctypes arrays of one comic_cnn_backward call; keeps every tensor alive until the call has run"""

    def __init__(self, ops, bufs, gbufs, chans, scales, grads, B, plan):
        self.n = len(ops)
        self.ops = (L.CnnOp * self.n)(*ops)
        self.keep = (bufs, gbufs, scales, grads)
        self.bufs = (C.c_void_p * len(bufs))(*[None if b is None else b.data_ptr() for b in bufs])
        self.gbufs = (C.c_void_p * len(gbufs))(*[None if b is None else b.data_ptr() for b in gbufs])
        self.chans = (C.c_int32 * len(chans))(*chans)
        self.wts = (L.ConvWeight * max(1, len(scales)))()
        for i, s in enumerate(scales):
            self.wts[i].scale = s.data_ptr()
        self.grads = (L.ConvGrad * max(1, len(grads)))()
        for i, gr in enumerate(grads):
            self.grads[i].w_master = gr['w'].data_ptr()
            self.grads[i].dw = gr['dw'].data_ptr()
            self.grads[i].dbeta = gr['dbeta'].data_ptr()
            self.grads[i].w_bwd = gr['wb'].data_ptr() if gr.get('wb') is not None else None
            self.grads[i].bwd_tile = gr.get('tile', 0)
        self.B, self.code = B, _CODE[plan]
        self.scratch_bytes = max(256, int(lib().comic_cnn_backward_scratch_bytes(self.ops, self.n, B, self.code, 1)))
        self.scratch = torch.full((self.scratch_bytes,), 0xFF, dtype=torch.uint8, device=DEV)

    def run(self, ready=0, code=None):
        L.check(lib().comic_cnn_backward(self.ops, self.n, self.bufs, self.gbufs, self.chans, self.wts, self.grads, self.B,
                                         self.code if code is None else code, ready, self.scratch.data_ptr(),
                                         self.scratch_bytes, stream(), None), 'cnn_backward')
        sync()

    def pack(self):
        L.check(lib().comic_cnn_pack_bwd_filters(self.ops, self.n, self.grads, self.code, stream()), 'pack_bwd_filters')
        sync()


def conv_op(g, plan, stem=False, src_coff=0, dst_coff=0, out_f32=0, src=0, dst=1, weight=0):
    x3 = plan == 'x3'
    return L.CnnOp(kind=1 if stem else 0, src=src, dst=dst, src_coff=src_coff, dst_coff=dst_coff, H=g.H, W=g.W,
                   Cin=g.Cin * (3 if x3 and not stem else 1), Cout=g.Cout, KH=g.KH, KW=g.KW, SH=g.S, SW=g.S, PT=g.PT, PL=g.PL,
                   Ho=g.Ho, Wo=g.Wo, weight=weight, relu=1, out_f32=out_f32, flags=L.OP_X3 if x3 else 0)


def conv_setup(name, case, ops, tile=0):
    """device buffers of one single-conv case, every accumulated buffer prefilled -> (Plan, dict of tensors and prefills)"""
    g, plan, stem = case['g'], case['plan'], case['stem']
    s = R.seed_of(name)
    K = g.KH * g.KW * g.Cin
    xd = f32_dev(ops['x']) if stem else act_dev(ops['x'], plan)
    t = dict(x=xd, y=act_dev(ops['y'], plan), dy=grad_dev(ops['dy'], plan), scale=f32_dev(ops['scale']), w=f32_dev(ops['w']))
    pf = dict(dw=R.prefill(s + 1, (K, g.Cout) if stem else (g.Cout, R.kpad(K))), dbeta=R.prefill(s + 2, (g.Cout,)))
    t['dw'], t['dbeta'] = f32_dev(pf['dw']), f32_dev(pf['dbeta'])
    gx = None
    if case['dgrad']:
        pf['gx'] = R.prefill(s + 3, (g.B, g.H, g.W, case['xc']), 'bf16' if plan == 'bf16' else 'f32')
        gx = t['gx'] = grad_dev(pf['gx'], plan)
        r = 3 if plan == 'x3' else 1
        t['wb'] = torch.full((g.Cin * R.kpad(g.KH * g.KW * r * g.Cout) * _ES[plan],), 0xFF, dtype=torch.uint8, device=DEV)
    xc = 3 if stem else case['xc'] * (3 if plan == 'x3' else 1)
    yc = g.Cout * (3 if plan == 'x3' else 1)
    pl = Plan([conv_op(g, plan, stem, case['src_coff'])], [t['x'], t['y']], [gx, t['dy']], [xc, yc], [t['scale']],
              [dict(w=t['w'], dw=t['dw'], dbeta=t['dbeta'], wb=t.get('wb'), tile=tile)], g.B, plan)
    return pl, t, pf


def packed(t, case):
    g, plan = case['g'], case['plan']
    r = 3 if plan == 'x3' else 1
    return host(t.view(_TDT[plan]).view(g.Cin, R.kpad(g.KH * g.KW * r * g.Cout)))


# ------------------------------------------------------------------------------------------------- activation gradient
ACT_FORMS = ['f32', 'bf16', 'bf16-f32y', 'x3', 'x3-f32y']


@pytest.mark.parametrize('form', ACT_FORMS)
@pytest.mark.parametrize('name', sorted(R.ACT_CASES))
def test_act_grad(name, form):
    """act_grad_kernel<float / bf16> and act_grad_x3_kernel (with bf16 regions and with an fp32 y): dz from the caller's
    scratch bit for bit, the zeros between dilated pixels included; d beta added to its prefill.  The op is a 1x1 conv of 8
    channels whose source has no gradient buffer: activation gradient and weight gradient are all that runs."""
    plan, f32y = form.split('-')[0], form.endswith('f32y')
    B, Ho, Wo, Cc, yc, coff, S = R.ACT_CASES[name]
    s = R.seed_of(name)
    print('\n%s %s: P = %d, C = %d at %d of %d, stride %d' % (name, form, B * Ho * Wo, Cc, coff, yc, S))
    yplan = 'f32' if f32y else plan
    y, dy, sc = R.make_y(s, (B, Ho, Wo, Cc), yplan), R.make_dy(s, (B, Ho, Wo, Cc), yplan if plan != 'x3' else 'x3'), R.make_scale(s, Cc)
    g = R.geo(B, (Ho - 1) * S + 1, (Wo - 1) * S + 1, 8, Cc, (1, 1), S, 'VALID')
    assert (g.Ho, g.Wo) == (Ho, Wo)
    x = R.make_x(s, (B, g.H, g.W, 8), plan)
    nan = float('nan')
    yd = f32_dev(wide(y, yc, coff, nan)) if f32y else act_dev(wide(y, yc, coff, nan), plan)
    dyd = f32_dev(wide(dy, yc, coff, nan)) if (f32y or plan == 'x3') else grad_dev(wide(dy, yc, coff, nan), plan)
    K = 8
    pf_dw, pf_db = R.prefill(s + 1, (Cc, 64)), R.prefill(s + 2, (Cc,))
    dw, db = f32_dev(pf_dw), f32_dev(pf_db)
    yc_phys = yc * (3 if plan == 'x3' and not f32y else 1)
    pl = Plan([conv_op(g, plan, dst_coff=coff, out_f32=int(f32y))], [act_dev(x, plan), yd], [None, dyd],
              [8 * (3 if plan == 'x3' else 1), yc_phys], [f32_dev(sc)], [dict(w=f32_dev(np.zeros((Cc, 64))), dw=dw, dbeta=db)], B, plan)
    pl.run()
    dz_ref, db_ref = R.act_grad(y, dy, sc, plan, S)
    same_bits(scratch_view(pl.scratch, 0, dz_ref.shape, plan), dz_ref, 'dz')
    tail = pl.scratch[dz_ref.size * _ES[plan]:]
    if S == 1 and tail.numel():                # (stride 2: the memset clears the slice's 256-byte rounding too)
        assert int(tail.min()) == 0xFF
    r32 = np.where(y > 0, dy, np.float32(0)).sum((0, 1, 2), dtype=np.float32)
    chk('d beta', host(db) - pf_db, db_ref, R.F32_BAR, R.rel_err(r32, db_ref))
    dzv = R.logical(dz_ref[:, ::S, ::S], plan)
    dw_ref = R.conv_wgrad(x, dzv, g)
    chk('dw (1x1, K = 8)', (host(dw) - pf_dw)[:, :K], dw_ref[:, :K], R.X3_BAR if plan == 'x3' else R.F32_BAR,
        R.rel_err(R.conv_wgrad(x, dzv, g, dtype=np.float32), dw_ref))
    same_bits(host(dw)[:, K:], pf_dw[:, K:], 'dw padding columns')


# ------------------------------------------------------------------------------------------------- one conv ----------
@pytest.mark.parametrize('name', sorted(CONV_CASES))
def test_conv_backward(name):
    """One conv through comic_cnn_backward: dz, d beta, dw (the four conv_wgrad_tr_kernel forms on bf16 and x3 plans, the fp32
    kernel, the stem kernel with its [K][Cout] layout), the packed backward-data filter and gx, at one and at three pixel
    splits and over the geometries of the network; then the same with the filters packed ahead by the table launch."""
    case = CONV_CASES[name]
    g, plan, stem = case['g'], case['plan'], case['stem']
    K, P = g.KH * g.KW * g.Cin, g.B * g.Ho * g.Wo
    print('\n%s: P = %d, K = %d (Kpad %d), Cout = %d, %dx%d / %d, source slice %d + %d of %d' % (
        name, P, K, R.kpad(K), g.Cout, g.KH, g.KW, g.S, case['src_coff'], g.Cin, case['xc']))
    ops = R.conv_operands(name, case)
    ref, r32 = R.conv_reference(case, ops), R.conv_reference(case, ops, np.float32)
    dw_bar, gx_bar, _ = R.conv_bars(case)
    pl, t, pf = conv_setup(name, case, ops)
    pl.run(ready=0)
    same_bits(scratch_view(pl.scratch, 0, ref['dz'].shape, plan), ref['dz'], 'dz')
    db32 = np.where(ops['y'] > 0, ops['dy'], np.float32(0)).sum((0, 1, 2), dtype=np.float32)
    chk('d beta', host(t['dbeta']) - pf['dbeta'], ref['dbeta'], R.F32_BAR, R.rel_err(db32, ref['dbeta']))
    got_dw = host(t['dw'])
    cols = slice(None) if stem else slice(0, K)
    chk('dw', (got_dw - pf['dw'])[:, cols], ref['dw'][:, cols], dw_bar, R.rel_err(r32['dw'], ref['dw']))
    if not stem:
        same_bits(got_dw[:, K:], pf['dw'][:, K:], 'dw padding columns [K, Kpad)')
    if not case['dgrad']:
        return
    same_bits(packed(t['wb'], case), ref['wb'], 'w_bwd (packed inline)')
    sl = slice(case['src_coff'], case['src_coff'] + g.Cin)
    got_gx = host(t['gx'])
    rest = R.rel_err(r32['gx'], ref['gx'])
    if plan == 'bf16':
        chk_bf16_store('gx = bf16(prefill + result)', got_gx[..., sl], pf['gx'][..., sl], ref['gx'], rest)
    else:
        chk('gx - prefill', got_gx[..., sl] - pf['gx'][..., sl], ref['gx'], gx_bar, rest)
    keep = np.ones(case['xc'], bool)
    keep[sl] = False
    same_bits(got_gx[..., keep], pf['gx'][..., keep], 'gx outside the slice')
    # filters packed ahead by the table launch, filters_ready = 1: the same filter and the same gx, bit for bit
    pl2, t2, _ = conv_setup(name, case, ops)
    pl2.pack()
    same_bits(packed(t2['wb'], case), ref['wb'], 'w_bwd (table launch)')
    pl2.run(ready=1)
    same_bits(host(t2['gx']), got_gx, 'gx with filters_ready = 1')


# ------------------------------------------------------------------------------------------------- backward-data ids --
@pytest.mark.parametrize('plan', ['bf16', 'f32', 'x3'])
@pytest.mark.parametrize('name', sorted(R.DGRAD_CASES))
def test_backward_data_accumulates_under_every_kernel_id(name, plan):
    """comic_conv_grad.bwd_tile picks the forward kernel of the backward-data convolution, which then runs with accum = 1: the
    read-modify-write epilogue of every id CnnEncoder.autotune_backward may choose.  Every im2col id must run, a patch-resident
    id may refuse the layer; every id that runs gives the bits of id 0, and id 0 is compared with float64 (x3: id 0 only, its
    backward-data conv runs on the heuristic tile)."""
    case = R.dgrad_case(name, plan)
    g = case['g']
    ops = R.conv_operands(name, case)
    ref, r32 = R.conv_reference(case, ops), R.conv_reference(case, ops, np.float32)
    print('\n%s %s' % (name, plan))
    base, ran, refused = None, [], []
    ids = [0] if plan == 'x3' else [i for i in range(0, L.IMG_TILE) if i != L.WS_TILE]
    for tile in ids:
        pl, t, pf = conv_setup(name, case, ops, tile=tile)
        try:
            pl.run()
        except L.ComicHipError:
            if L.is_im2col_tile(tile):
                raise
            sync()
            refused.append(tile)
            continue
        ran.append(tile)
        got = host(t['gx'])
        if base is None:
            base = got
            rest = R.rel_err(r32['gx'], ref['gx'])
            if plan == 'bf16':
                chk_bf16_store('id 0: gx = bf16(prefill + result)', got, pf['gx'], ref['gx'], rest)
                # every element written exactly once: never the prefill alone, never twice the contribution
                for wrong, what in ((pf['gx'], 'not written'), (pf['gx'] + 2 * ref['gx'], 'added twice')):
                    assert R.rel_err(got, R.bf16_round(np.asarray(wrong, np.float32))) > 10 * R.BF16_STORE_BAR, what
            else:
                chk('id 0: gx - prefill', got - pf['gx'], ref['gx'], R.conv_bars(case)[1], rest)
            assert len(np.unique(pf['gx'])) > (100 if plan == 'bf16' else got.size // 2)       # distinct prefill values
        else:
            np.testing.assert_array_equal(R.bits(got), R.bits(base), err_msg='kernel id %d' % tile)
    print('  ids that ran, all with the bits of id 0: %s' % ran)
    print('  ids that refused the layer: %s' % refused)
    assert all(L.is_im2col_tile(i) or i in ran or i in refused for i in ids)
    assert [i for i in ids if L.is_im2col_tile(i)] == [i for i in ran if L.is_im2col_tile(i)]


# ------------------------------------------------------------------------------------------------- fused act gradient -
def sched_run(ops_, bufs, gbufs, chans, scales, grads, B, plan, flags, lanes):
    pl = Plan(ops_, bufs, gbufs, chans, scales, grads, B, plan)
    nbytes = int(lib().comic_cnn_backward_scratch_bytes(pl.ops, pl.n, B, pl.code, 2))
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    sched = np.ascontiguousarray([[0, i, 0, 0] for i in range(pl.n - 1, -1, -1)], np.int32)
    sync()
    L.check(lib().comic_cnn_backward_sched(pl.ops, pl.n, sched.ctypes.data, len(sched), pl.bufs, pl.gbufs, None, pl.chans, pl.wts,
                                           pl.grads, B, pl.code, flags, scratch.data_ptr(), nbytes, stream(),
                                           lanes[0].cuda_stream, lanes[1].cuda_stream), 'cnn_backward_sched')
    sync()
    return scratch


def chain_run(o, plan, fused, g1_prefill):
    """the chain p -> c of R.fused_operands on one plan -> dz_p, dz_c (from the scratch, slices in op order), g1 (the gradient
    buffer between the two convs), dw_p, dw_c, dbeta_p and their prefills"""
    gp, gc = o['gp'], o['gc']
    s = R.seed_of('chain')
    Cc = gp.Cout
    pf = dict(dw_p=R.prefill(s + 1, (Cc, R.kpad(gp.KH * gp.KW * 32))), dw_c=R.prefill(s + 2, (64, R.kpad(9 * Cc))),
              db_p=R.prefill(s + 3, (Cc,)), db_c=R.prefill(s + 4, (64,)), g1=g1_prefill)
    t = {k: f32_dev(v) for k, v in pf.items() if k != 'g1'}
    t['g1'] = grad_dev(pf['g1'], plan)
    wb_c = torch.full((Cc * R.kpad(9 * 64) * _ES[plan],), 0xFF, dtype=torch.uint8, device=DEV)
    lanes = (torch.cuda.Stream(), torch.cuda.Stream())
    ops_ = [conv_op(gp, plan, src=0, dst=1, weight=0), conv_op(gc, plan, src=1, dst=2, weight=1)]
    bufs = [act_dev(o['x_p'], plan), act_dev(o['y_p'], plan), act_dev(o['y_c'], plan)]
    gbufs = [None, t['g1'], grad_dev(o['dy_c'], plan)]
    grads = [dict(w=f32_dev(o['w_p']), dw=t['dw_p'], dbeta=t['db_p']), dict(w=f32_dev(o['w_c']), dw=t['dw_c'], dbeta=t['db_c'], wb=wb_c)]
    scratch = sched_run(ops_, bufs, gbufs, [32, Cc, 64], [f32_dev(o['scale_p']), f32_dev(o['scale_c'])], grads, gp.B, plan,
                        0 if fused else L.CNN_BWD_NO_ACT_FUSION, lanes)
    dzp_shape = (gp.B, (gp.Ho - 1) * gp.S + 1, (gp.Wo - 1) * gp.S + 1, Cc)
    n_p = int(np.prod(dzp_shape)) * _ES[plan]
    out = dict(dz_p=scratch_view(scratch, 0, dzp_shape, plan),
               dz_c=scratch_view(scratch, (n_p + 255) // 256 * 256, (gc.B, gc.Ho, gc.Wo, 64), plan))
    out.update({k: host(v) for k, v in t.items()})
    return out, pf


@pytest.mark.parametrize('Cc', R.FUSED_C)
def test_fused_activation_gradient(Cc):
    """comic_cnn_backward_sched on the chain p (1x1, 32 -> C) -> c (3x3, C -> 64): c's backward-data launch applies p's
    activation gradient in its epilogue (conv_store_tiles<MASK> on the bf16 plan, the fp32 kernel's MASK branch on the fp32
    plan), writes p's dz and the kMaskCopies partial d beta rows, and dbeta_fold_kernel adds them to d beta.  The accumulators are
    exact by construction (R.fused_operands), so the unfused fp32 plan's gradient buffer IS the accumulator tensor and dz_p is
    compared bit for bit."""
    o = R.fused_operands(Cc, 'bf16')
    gp, gc = o['gp'], o['gc']
    print('\nfused chain, C = %d, %d pixels' % (Cc, gp.B * gp.Ho * gp.Wo))
    zeros = np.zeros((gp.B, gp.Ho, gp.Wo, Cc), np.float32)
    nonzero = R.prefill(11, zeros.shape, 'bf16')
    dz_c, dbeta_c = R.act_grad(o['y_c'], o['dy_c'], o['scale_c'], 'bf16')
    g_exact = R.conv_dgrad(dz_c, o['w_c'], gc)
    # the device's own accumulators: the unfused fp32 plan, gradient buffer zero before the launch
    u32, _ = chain_run(o, 'f32', False, zeros)
    same_bits(u32['g1'], g_exact.astype(np.float32), 'fp32 plan, unfused: g (accumulators of the backward-data launch)')
    g = u32['g1']
    dwc_ref, dwc_32 = R.conv_wgrad(o['y_p'], dz_c, gc), R.conv_wgrad(o['y_p'], dz_c, gc, dtype=np.float32)
    for plan in ('bf16', 'f32'):
        f, pf = chain_run(o, plan, True, nonzero)
        dzp_ref, dbp_ref = R.fused_act_grad(g, o['y_p'], o['scale_p'], plan)
        same_bits(f['dz_c'], dz_c, '%s fused: dz_c' % plan)
        same_bits(f['dz_p'], dzp_ref, '%s fused: dz_p (MASK epilogue)' % plan)
        same_bits(f['g1'], nonzero, '%s fused: gradient buffer between the convs untouched' % plan)
        db32 = np.where(o['y_p'] > 0, g, np.float32(0)).sum((0, 1, 2), dtype=np.float32)
        chk('%s fused: d beta_p - prefill (dbeta_fold)' % plan, f['db_p'] - pf['db_p'], dbp_ref, R.F32_BAR, R.rel_err(db32, dbp_ref))
        chk('%s fused: d beta_c - prefill' % plan, f['db_c'] - pf['db_c'], dbeta_c, R.F32_BAR, 0.0)
        dwp_ref = R.conv_wgrad(o['x_p'], dzp_ref, gp)
        Kp, Kc = 32, 9 * Cc
        chk('%s fused: dw_p' % plan, (f['dw_p'] - pf['dw_p'])[:, :Kp], dwp_ref[:, :Kp], R.F32_BAR,
            R.rel_err(R.conv_wgrad(o['x_p'], dzp_ref, gp, dtype=np.float32), dwp_ref))
        chk('%s fused: dw_c' % plan, (f['dw_c'] - pf['dw_c'])[:, :Kc], dwc_ref[:, :Kc], R.F32_BAR, R.rel_err(dwc_32, dwc_ref))
        same_bits(f['dw_p'][:, Kp:], pf['dw_p'][:, Kp:], '%s fused: dw_p padding columns' % plan)
        # the unfused chain of the same plan: p's act_grad launch reads the stored gradient buffer
        u, _ = chain_run(o, plan, False, zeros)
        g_stored = R.bf16_round(g) if plan == 'bf16' else g
        same_bits(u['g1'], g_stored, '%s unfused: g as stored' % plan)
        same_bits(u['dz_p'], R.act_grad(o['y_p'], g_stored, o['scale_p'], plan)[0], '%s unfused: dz_p' % plan)
        if plan == 'bf16':
            moved = int((R.bits(u['dz_p']) != R.bits(f['dz_p'])).sum())
            print('  bf16: %d of %d dz_p values differ between the fused and the unfused run' % (moved, u['dz_p'].size))
            assert moved > 0                        # the fused form did run: it skips the rounding of the stored gradient


def test_activation_gradient_is_not_fused_across_a_stride():
    """p with stride 2 must not fuse (a fused epilogue writes an undilated dz): with and without COMIC_CNN_BWD_NO_ACT_FUSION
    the call gives the unfused result, bit for bit where the result does not depend on the order of atomics"""
    o = R.fused_operands(48, 'bf16', p_stride=2)
    gc = o['gc']
    zeros = np.zeros((gc.B, gc.H, gc.W, 48), np.float32)
    dz_c, _ = R.act_grad(o['y_c'], o['dy_c'], o['scale_c'], 'bf16')
    g_stored = R.bf16_round(R.conv_dgrad(dz_c, o['w_c'], gc).astype(np.float32))
    want = R.act_grad(o['y_p'], g_stored, o['scale_p'], 'bf16', 2)[0]
    print()
    outs = []
    for fused in (True, False):
        f, _ = chain_run(o, 'bf16', fused, zeros)
        same_bits(f['g1'], g_stored, 'fusion %s: g as stored' % ('allowed' if fused else 'off'))
        same_bits(f['dz_p'], want, 'fusion %s: dz_p (zero-dilated)' % ('allowed' if fused else 'off'))
        outs.append(f)
    chk('dw_p, fusion allowed against fusion off', outs[0]['dw_p'], outs[1]['dw_p'], R.F32_BAR, 0.0)


# ------------------------------------------------------------------------------------------------- pools --------------
def _pool_forms(kind):
    return ['f32', 'bf16', 'bf16-srcf32'] if kind == 4 else ['f32', 'bf16', 'x3']


POOL_PARAMS = [(n, f, t) for n in sorted(R.POOL_CASES) for f in _pool_forms(R.POOL_CASES[n][0])
               for t in ((False, True) if R.POOL_CASES[n][0] == 2 else (False,))]


@pytest.mark.parametrize('name,form,ties', POOL_PARAMS)
def test_pool_backward(name, form, ties):
    """maxpool_grad_s2_kernel (plain and x3: 16 x 16 LDS tiles, one tile plus one pixel, ragged chunk groups, padding as -inf,
    tied maxima) and the three modes of pool_grad_kernel, each into a prefilled slice of a wider gradient buffer.  The max-pool
    gradients are sums of at most four dy in (ho, wo) order: the float32 restatement in that order is compared bit for bit --
    for the tiled and the gather kernel alike, which is the claim that the two give identical bits."""
    case = R.POOL_CASES[name]
    kind, g = case[0], R.pool_geo(case)
    plan = form.split('-')[0]
    src_f32 = form.endswith('srcf32')
    x3 = plan == 'x3'
    Cc = g.Cin
    xcl, xoff, ycl, yoff = Cc + 16, 8, Cc + 8, 8                # logical channels of the buffers, the op's slices
    x, dy = R.pool_operands(name, case, plan, ties)
    print('\n%s %s%s: %dx%d -> %dx%d, C = %d' % (name, form, ' ties' if ties else '', g.H, g.W, g.Ho, g.Wo, Cc))
    dy_f32 = kind == 4 or x3 or plan == 'f32'
    dx_f32 = plan == 'f32' or x3 or src_f32
    nan = float('nan')
    xd = act_dev(wide(x, xcl, xoff, nan), plan)
    dyd = f32_dev(wide(dy, ycl, yoff, nan)) if dy_f32 else grad_dev(wide(dy, ycl, yoff, nan), 'bf16')
    pf = R.prefill(R.seed_of(name) + 9, (g.B, g.H, g.W, xcl), 'f32' if dx_f32 else 'bf16')
    dxd = f32_dev(pf) if dx_f32 else grad_dev(pf, 'bf16')
    op = L.CnnOp(kind=kind, src=0, dst=1, src_coff=xoff, dst_coff=yoff, H=g.H, W=g.W, Cin=Cc, Cout=Cc, KH=g.KH, KW=g.KW, SH=g.S,
                 SW=g.S, PT=g.PT, PL=g.PL, Ho=g.Ho, Wo=g.Wo, weight=-1, relu=0, out_f32=int(kind == 4), src_f32=int(src_f32),
                 flags=L.OP_X3 if x3 else 0)
    m = 3 if x3 else 1
    pl = Plan([op], [xd, dyd], [dxd, dyd], [xcl * m, ycl * m], [], [], g.B, plan)
    pl.run()
    got = host(dxd)
    sl = slice(xoff, xoff + Cc)
    ref, r32 = R.pool_reference(case, x, dy), R.pool_reference(case, x, dy, np.float32)
    rest = R.rel_err(r32, ref)
    if dx_f32:
        chk('dx - prefill', got[..., sl] - pf[..., sl], ref, R.F32_BAR, rest)
    else:
        chk_bf16_store('dx = bf16(prefill + result)', got[..., sl], pf[..., sl], ref, rest)
    if kind == 2:
        want = pf[..., sl] + r32                                  # float32: old + (the windows' dy added in (ho, wo) order)
        same_bits(got[..., sl], want if dx_f32 else R.bf16_round(want), 'dx against the float32 sums in (ho, wo) order')
    keep = np.ones(xcl, bool)
    keep[sl] = False
    same_bits(got[..., keep], pf[..., keep], 'dx outside the slice')


# ------------------------------------------------------------------------------------------------- refusals -----------
def _small_conv(plan, cin=32, stride=1, dst_coff=0, yc=None, name='refusal'):
    g = R.geo(2, 9, 9, cin, 32, (3, 3), stride, 'SAME' if stride == 1 else 'VALID')
    case = dict(plan=plan, g=g, xc=cin, src_coff=0, stem=False, dgrad=True)
    ops = R.conv_operands(name, case)
    return case, ops


def _unchanged(t, pf, what):
    for k in ('dw', 'dbeta', 'gx'):
        same_bits(host(t[k]), pf[k], '%s: %s as prefilled' % (what, k))


def test_refusals():
    """calls that must return an error, and leave dw, d beta and gx as they were"""
    print()
    case, ops = _small_conv('bf16')
    # the f16 dtype has no backward
    pl, t, pf = conv_setup('refusal', case, ops)
    with pytest.raises(L.ComicHipError):
        pl.run(code=2)
    with pytest.raises(L.ComicHipError):
        L.check(lib().comic_cnn_pack_bwd_filters(pl.ops, 1, pl.grads, 2, stream()))
    assert lib().comic_cnn_backward_scratch_bytes(pl.ops, 1, 2, 2, 1) == -1
    lanes = (torch.cuda.Stream(), torch.cuda.Stream())
    sched = np.ascontiguousarray([[0, 0, 0, 0]], np.int32)
    with pytest.raises(L.ComicHipError):
        L.check(lib().comic_cnn_backward_sched(pl.ops, 1, sched.ctypes.data, 1, pl.bufs, pl.gbufs, None, pl.chans, pl.wts, pl.grads, 2,
                                               2, 0, pl.scratch.data_ptr(), pl.scratch_bytes, stream(), lanes[0].cuda_stream,
                                               lanes[1].cuda_stream))
    sync()
    _unchanged(t, pf, 'f16')
    # a schedule that names an op twice
    twice = np.ascontiguousarray([[0, 0, 0, 0], [0, 0, 0, 0]], np.int32)
    nbytes = int(lib().comic_cnn_backward_scratch_bytes(pl.ops, 1, 2, 1, 2))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    with pytest.raises(L.ComicHipError):
        L.check(lib().comic_cnn_backward_sched(pl.ops, 1, twice.ctypes.data, 2, pl.bufs, pl.gbufs, None, pl.chans, pl.wts, pl.grads, 2,
                                               1, 0, scratch.data_ptr(), nbytes, stream(), lanes[0].cuda_stream, lanes[1].cuda_stream))
    sync()
    # stride 3
    pl, t, pf = conv_setup('refusal', case, ops)
    pl.ops[0].SH = pl.ops[0].SW = 3
    with pytest.raises(L.ComicHipError):
        pl.run()
    _unchanged(t, pf, 'stride 3')
    # a misaligned output slice (bf16: 8-channel chunks)
    pl, t, pf = conv_setup('refusal', case, ops)
    pl.ops[0].dst_coff = 4
    with pytest.raises(L.ComicHipError):
        pl.run()
    _unchanged(t, pf, 'misaligned slice')
    # a conv whose backward-data convolution the forward kernels refuse (they need Cout % 16 == 0, here the conv's Cin): the
    # call must refuse in front of its first launch, not after the activation and weight gradients have been added
    for plan, cin in (('bf16', 40), ('x3', 40), ('f32', 24)):
        case, ops = _small_conv(plan, cin, name='refusal%d' % cin)
        pl, t, pf = conv_setup('refusal', case, ops)
        with pytest.raises(L.ComicHipError):
            pl.run()
        _unchanged(t, pf, '%s, Cin %d' % (plan, cin))
        assert int(pl.scratch.min()) == 0xFF          # not even dz was written
        # ... while the same conv without a source gradient buffer (weight gradient only) runs
        case2 = dict(case, dgrad=False)
        pl, t, pf = conv_setup('refusal', case2, ops)
        pl.run()
        ref, r32 = R.conv_reference(case2, ops), R.conv_reference(case2, ops, np.float32)
        K = 9 * cin
        chk('%s, Cin %d, no source gradient: dw' % (plan, cin), (host(t['dw']) - pf['dw'])[:, :K], ref['dw'][:, :K],
            R.conv_bars(case2)[0], R.rel_err(r32['dw'], ref['dw']))
