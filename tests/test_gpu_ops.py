"""Op-level parity: every HIP kernel behind the C-ABI vs the CPU oracle on the same seeded
inputs.  Tolerances: fp32 1e-3 relative (max-norm), bf16 storage 2e-2 vs a bf16-emulating
oracle (inputs/weights rounded to bf16, fp32 accumulate), indices bit-exact.
The decoder ops here run with every executor-only argument null, 0 or 1; the forms the executors launch (split
attention, fused epilogue, shared memories, split backward, fused losses, LN_LSTM / GRU cells, split-K partials) are in
tests/test_gpu_exec_ops.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import comic_amd._lib as L
from oracle import beam_ref, cnn_ref, decoder_ref as dr
from tests import exec_ops_ref, regimes
from tests.gpu_util import DEV, F32_RTOL, P, assert_close, dev, elementwise_excess, lib, rel_err, stream, sync


# ------------------------------------------------------------------------ GEMM -----------
@pytest.mark.parametrize('M,N,K,ta,tb', [
    (64, 2048, 1280, 0, 0), (64, 512, 512, 0, 0), (64, 258, 512, 0, 0), (37, 258, 130, 0, 0),
    (64, 1280, 2048, 0, 1), (64, 512, 258, 0, 1), (1856, 512, 258, 0, 1),
    (1280, 2048, 1856, 1, 0), (512, 258, 1856, 1, 0), (2048, 768, 64, 1, 0), (33, 70, 19, 1, 1),
    (1600, 512, 2048, 0, 0), (2048, 512, 1600, 1, 0)])
def test_gemm_f32(M, N, K, ta, tb):
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((K, M) if ta else (M, K)).astype(np.float32)
    B = rng.standard_normal((N, K) if tb else (K, N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    C0 = rng.standard_normal((M, N)).astype(np.float32)
    ref = (A.T if ta else A).astype(np.float64) @ (B.T if tb else B).astype(np.float64)
    dA, dB, dC, db = dev(A), dev(B), dev(C0), dev(bias)
    L.check(lib().comic_gemm_f32(dA.data_ptr(), dB.data_ptr(), dC.data_ptr(), db.data_ptr(), M, N, K,
                                 A.shape[1], B.shape[1], N, ta, tb, 0.5, 2.0, stream()))
    sync()
    assert_close(dC.cpu().numpy(), 0.5 * ref + 2.0 * C0 + bias, 1e-5, 'gemm')
    # plain product, strided C (ldc > N)
    big = torch.zeros((M, N + 8), dtype=torch.float32, device=DEV)
    L.check(lib().comic_gemm_f32(dA.data_ptr(), dB.data_ptr(), big.data_ptr(), None, M, N, K, A.shape[1],
                                 B.shape[1], N + 8, ta, tb, 1.0, 0.0, stream()))
    sync()
    assert_close(big[:, :N].cpu().numpy(), ref, 1e-5, 'gemm strided')
    assert float(big[:, N:].abs().max()) == 0.0


@pytest.mark.parametrize('R,K,N', [(150, 512, 512), (33, 96, 70), (256, 1000, 258), (64, 2816, 2048), (224, 512, 258),
                                   (100, 40, 1), (35, 520, 130)])
def test_gemm_f32_stream(R, K, N):
    """Weight-streaming skinny product of the decode steps (csrc/lstm_stream.hip through its C-ABI entry): rows on one and
    two 16-row tiles per wave and with idle waves, K not a multiple of the 32-deep step, N not a multiple of the
    64-column chunk, the LSTM gate product's shape; bf16 hi/lo split products, bound 5e-5 of the result's max-norm."""
    rng = np.random.default_rng(R + K + N)
    x = rng.standard_normal((R, K)).astype(np.float32)
    W = rng.standard_normal((K, N)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    ref = x.astype(np.float64) @ W.astype(np.float64) + b
    nb = int(lib().comic_gemm_f32_stream_workspace(R, K, N))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    dx, dW, db = dev(x), dev(W), dev(b)
    out = torch.full((R, N), float('nan'), dtype=torch.float32, device=DEV)
    for _ in range(3):
        L.check(lib().comic_gemm_f32_stream(dx.data_ptr(), dW.data_ptr(), db.data_ptr(), out.data_ptr(), R, K, N,
                                            ws.data_ptr(), nb, stream()))
    sync()
    assert_close(out.cpu().numpy(), ref, 5e-5, 'gemm stream')
    out2 = torch.empty_like(out)
    L.check(lib().comic_gemm_f32_stream(dx.data_ptr(), dW.data_ptr(), None, out2.data_ptr(), R, K, N, ws.data_ptr(), nb,
                                        stream()))
    sync()
    assert_close(out2.cpu().numpy(), ref - b, 5e-5, 'gemm stream, no bias')
    with pytest.raises(L.ComicHipError):
        L.check(lib().comic_gemm_f32_stream(dx.data_ptr(), dW.data_ptr(), None, out2.data_ptr(), 16, K, N, ws.data_ptr(), nb,
                                            stream()))


@pytest.mark.parametrize('M,N,K,ta,tb', [
    (1600, 512, 2048, 0, 0), (1856, 258, 512, 0, 0), (1856, 512, 258, 0, 1), (1280, 2048, 1856, 1, 0),
    (512, 258, 1856, 1, 0), (2048, 512, 1600, 1, 0), (33, 70, 19, 1, 1), (130, 131, 45, 0, 1), (257, 129, 64, 0, 0),
    # decode-step shapes: all rows in one 160- / 192-row tile over a wide (unaligned / aligned) vocabulary
    (150, 8195, 512, 0, 0), (150, 8196, 96, 0, 1), (190, 8200, 100, 0, 0), (161, 8300, 64, 1, 0)])
def test_gemm_f32_split3(M, N, K, ta, tb):
    """bf16 hi/lo split products (hi*hi + hi*lo + lo*hi, fp32 accumulate): every layout, ragged tiles,
    alpha/beta/bias and a strided C; error bound 5e-5 of the result's max-norm (measured ~2e-6)."""
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((K, M) if ta else (M, K)).astype(np.float32)
    B = rng.standard_normal((N, K) if tb else (K, N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    C0 = rng.standard_normal((M, N)).astype(np.float32)
    ref = (A.T if ta else A).astype(np.float64) @ (B.T if tb else B).astype(np.float64)
    dA, dB, dC, db = dev(A), dev(B), dev(C0), dev(bias)
    L.check(lib().comic_gemm_f32_split3(dA.data_ptr(), dB.data_ptr(), dC.data_ptr(), db.data_ptr(), M, N, K,
                                        A.shape[1], B.shape[1], N, ta, tb, 0.5, 2.0, None, 0, stream()))
    sync()
    assert_close(dC.cpu().numpy(), 0.5 * ref + 2.0 * C0 + bias, 5e-5, 'gemm split3')
    # with a workspace: split-K slabs for the shapes with few output tiles, same contract
    ws = torch.empty(8 << 20, dtype=torch.uint8, device=DEV)
    dC2 = dev(C0)
    L.check(lib().comic_gemm_f32_split3(dA.data_ptr(), dB.data_ptr(), dC2.data_ptr(), db.data_ptr(), M, N, K,
                                        A.shape[1], B.shape[1], N, ta, tb, 0.5, 2.0, ws.data_ptr(), 8 << 20, stream()))
    sync()
    assert_close(dC2.cpu().numpy(), 0.5 * ref + 2.0 * C0 + bias, 5e-5, 'gemm split3 + split-K')
    big = torch.zeros((M, N + 8), dtype=torch.float32, device=DEV)
    L.check(lib().comic_gemm_f32_split3(dA.data_ptr(), dB.data_ptr(), big.data_ptr(), None, M, N, K, A.shape[1],
                                        B.shape[1], N + 8, ta, tb, 1.0, 0.0, ws.data_ptr(), 8 << 20, stream()))
    sync()
    assert_close(big[:, :N].cpu().numpy(), ref, 5e-5, 'gemm split3 strided')
    assert float(big[:, N:].abs().max()) == 0.0


_GG_SPECS = {  # type, M, N, K, extras
    # any alignment: the four-wave kernel with scalar loads where rows are not 16-byte aligned
    'mixed': [
        (0, 1280, 2048, 1920, {}), (0, 2048, 512, 1600, {}), (2, 1856, 256, 2048, {'mask': 768}),
        (0, 512, 258, 1856, {}), (1, 1600, 512, 2048, {}), (1, 64, 768, 2048, {'mask': 768, 'ldc': 1280}),
        (0, 1, 2048, 1920, {'ones': True}), (0, 1, 258, 1856, {'ones': True}), (0, 1, 1, 256, {'ones': True, 'ldb': 1537}),
        (2, 64, 768, 2048, {'bias': True}), (0, 33, 70, 19, {'beta': 2.0}), (1, 130, 131, 45, {'bias': True, 'beta': -1.0}),
        (2, 257, 129, 64, {}), (1, 1856, 258, 512, {'bias': True})],
    # every operand row 16-byte aligned: the producer / consumer kernel (the training step's shapes, ragged tiles, short
    # and odd k-tile counts, N not a multiple of 4 inside a padded row)
    'aligned': [
        (0, 1280, 2048, 1920, {}), (0, 2048, 512, 1600, {}), (2, 1856, 256, 2048, {'mask': 768}),
        (0, 512, 258, 1856, {'ldb': 260}), (1, 1600, 512, 2048, {}), (1, 64, 768, 2048, {'mask': 768, 'ldc': 1280}),
        (0, 1, 2048, 1920, {'ones': True}), (0, 1, 258, 1856, {'ones': True, 'ldb': 260}), (0, 1, 1, 256, {'ones': True, 'ldb': 1537}),
        (2, 64, 768, 2048, {'bias': True}), (0, 36, 72, 20, {'beta': 2.0}), (1, 132, 130, 44, {'bias': True, 'beta': -1.0, 'ldb': 132}),
        (2, 257, 129, 64, {}), (1, 1856, 258, 512, {'bias': True, 'ldb': 260}), (2, 1856, 512, 260, {}), (1, 100, 100, 100, {}),
        (0, 100, 100, 300, {})],
}


@pytest.mark.parametrize('which', ['mixed', 'aligned'])
def test_gemm_group_matches_numpy_and_is_reproducible(which):
    """comic_gemm_group: the three operand layouts, bias / dropout-mask / beta epilogues, column sums as products, ragged
    tiles and split-K tiles combined inside the launch -- every problem against numpy in float64 (5e-5 of the
    max-norm, as comic_gemm_f32_split3), a second launch over the same buffers bit-equal to the first."""
    rng = np.random.default_rng(7)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    keep = 0.75
    specs = _GG_SPECS[which]
    probs = (L.GemmProb * len(specs))()
    keepalive, refs, outs = [], [], []
    for i, (ty, M, N, K, ex) in enumerate(specs):
        ones = ex.get('ones', False)
        ldb = ex.get('ldb', K if ty == 2 else N)
        A = None if ones else (f(K, M) if ty == 0 else f(M, K))
        Bfull = f(N, ldb) if ty == 2 else f(K, ldb)
        Bm = Bfull[:, :K].T if ty == 2 else Bfull[:, :N]
        Am = np.ones((1, K), np.float32) if ones else (A.T if ty == 0 else A)
        ref = Am.astype(np.float64) @ Bm.astype(np.float64)
        ldc = ex.get('ldc', N)
        C0 = f(M, ldc)
        if ex.get('bias'):
            bias = f(N); ref = ref + bias
        else:
            bias = None
        if 'mask' in ex:
            ldm = ex['mask']
            mask = (rng.uniform(size=(M, ldm)) < keep).astype(np.float32)
            ref = ref / keep * mask[:, :N]
        else:
            mask, ldm = None, 0
        beta = ex.get('beta', 0.0)
        ref = ref + beta * C0[:, :N]
        dA = None if ones else dev(A)
        dB, dC = dev(Bfull), dev(C0)
        db = dev(bias) if bias is not None else None
        dm = dev(mask) if mask is not None else None
        keepalive += [dA, dB, dC, db, dm]
        q = probs[i]
        q.A = dA.data_ptr() if dA is not None else None
        q.B, q.C = dB.data_ptr(), dC.data_ptr()
        q.bias = db.data_ptr() if db is not None else None
        q.mask = dm.data_ptr() if dm is not None else None
        q.M, q.N, q.K, q.lda, q.ldb, q.ldc, q.ld_mask = M, N, K, (1 if ones else A.shape[1]), ldb, ldc, ldm
        q.alpha, q.beta, q.keep, q.type, q.ones_a = 1.0, beta, keep, ty, int(ones)
        refs.append(ref); outs.append((dC, C0, N))
    nbytes = lib().comic_gemm_group_workspace(probs, len(specs))
    assert nbytes > 0
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=DEV)
    L.check(lib().comic_gemm_group(probs, len(specs), ws.data_ptr(), nbytes, stream()), 'gemm_group')
    sync()
    first = []
    for (dC, C0, N), ref, sp in zip(outs, refs, specs):
        got = dC.cpu().numpy()
        assert_close(got[:, :N], ref, 5e-5, 'gemm_group %r' % (sp[:4],))
        assert np.array_equal(got[:, N:], C0[:, N:]), 'gemm_group wrote outside its columns'
        first.append(got.copy())
    # second launch into fresh outputs: same bits (fixed-order combine), tickets left clean by the first
    for (dC, C0, N) in outs:
        dC.copy_(torch.from_numpy(C0))
    L.check(lib().comic_gemm_group(probs, len(specs), ws.data_ptr(), nbytes, stream()), 'gemm_group')
    sync()
    for (dC, _, _), a in zip(outs, first):
        assert np.array_equal(dC.cpu().numpy(), a)


# ------------------------------------------------------------------------ conv / pool -----
_TDT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
_CODE = {'f32': 0, 'bf16': 1, 'f16': 2}


def _run_conv(x, w, beta, mean, var, stride, padding, dtype, dst_channels=None, dst_coff=0, relu=1, out_f32=0, tile=0,
              flags=0):
    B, H, W, Cin = x.shape
    kh, kw, _, Cout = w.shape
    if flags & L.OP_POOLED_SRC:             # 1x1 conv behind a 3x3 / 2 VALID max-pool folded into its loads
        Ho, Wo, pt, pl = (H - 3) // 2 + 1, (W - 3) // 2 + 1, 0, 0
    else:
        Ho, pt, _ = cnn_ref.out_size(H, kh, stride, padding)
        Wo, pl, _ = cnn_ref.out_size(W, kw, stride, padding)
    tdt = _TDT[dtype]
    code = _CODE[dtype]
    stem = Cin <= 4
    xd = dev(x) if stem else dev(x).to(tdt)
    wd = dev(w)
    scale = torch.empty(Cout, device=DEV); shift = torch.empty(Cout, device=DEV)
    L.check(lib().comic_fold_bn(P(beta), P(mean), P(var), 1e-3,
                                scale.data_ptr(), shift.data_ptr(), Cout, stream()))
    if stem:
        packed = wd.reshape(-1, Cout).contiguous()
    else:
        K = kh * kw * Cin
        packed = torch.empty(Cout * ((K + 63) // 64 * 64), dtype=tdt, device=DEV)
        L.check(lib().comic_pack_conv_weights(wd.data_ptr(), packed.data_ptr(), kh, kw, Cin, Cout, code, stream()))
    yc = dst_channels or Cout
    ydt = torch.float32 if out_f32 else tdt
    y = torch.full((B, Ho, Wo, yc), -7.0, dtype=ydt, device=DEV)
    op = L.CnnOp(kind=1 if stem else 0, src=0, dst=1, src_coff=0, dst_coff=dst_coff, H=H, W=W, Cin=Cin, Cout=Cout,
                 KH=kh, KW=kw, SH=stride, SW=stride, PT=pt, PL=pl, Ho=Ho, Wo=Wo, weight=0, relu=relu, out_f32=out_f32,
                 tile=tile, flags=flags)
    wt = L.ConvWeight(packed.data_ptr(), scale.data_ptr(), shift.data_ptr())
    L.check(lib().comic_conv2d_bn_relu(C.byref(op), xd.data_ptr(), Cin, y.data_ptr(), yc, C.byref(wt), B, code,
                                       stream()), 'conv')
    sync()
    return y.float().cpu().numpy()


def _ref_conv(x, w, beta, mean, var, stride, padding, dtype, relu=1, round_out=True):
    """bf16: the bf16-emulating oracle (fp32 accumulate).  f16: float64 on the f16 operands the kernel reads (the
    stem: the fp32 image and filter), BatchNorm in float64, ONE rounding of the output to f16 -- what is left between
    kernel and reference is the kernel's fp32 accumulation and its single RNE store."""
    if dtype == 'f16':
        stem = x.shape[-1] <= 4
        q = (lambda a: np.asarray(a, np.float64)) if stem else (lambda a: cnn_ref.f16_round(np.asarray(a, np.float64)))
        y = cnn_ref.conv2d(q(x), q(w), stride, padding)
        y = (y - mean.astype(np.float64)) / np.sqrt(var.astype(np.float64) + cnn_ref.BN_EPS) + beta.astype(np.float64)
        if relu:
            y = np.maximum(y, 0)
        return cnn_ref.f16_round(y) if round_out else y
    q = cnn_ref.bf16_round if dtype == 'bf16' else (lambda a: a)
    y = cnn_ref.conv2d(q(x), q(w), stride, padding)
    y = cnn_ref.batch_norm_inference(y, beta, mean, var)
    if relu:
        y = np.maximum(y, 0)
    return q(y) if round_out else y


def _assert_f16(got, ref, name):
    """The f16 op bar: the north star's fp32 criterion (1e-3, max-norm AND element-wise) against the float64 reference.
    The bar must discriminate: the reference rounded through bf16 instead fails it, so a kernel that rounds through
    bf16 anywhere cannot pass.  (Outputs with fewer than 32 non-zero values -- the 1x1 map cases -- are exempt from that
    second check: a handful of bf16 roundings can all land close enough by chance.)"""
    assert_close(got, ref, F32_RTOL, name + ' f16', elementwise=True)
    if np.count_nonzero(ref) < 32:
        return
    with pytest.raises(AssertionError):
        assert_close(cnn_ref.bf16_round(np.asarray(ref, np.float32)), ref, F32_RTOL, name + ' bf16-rounded', elementwise=True)


def _check(got, ref, dtype, name, tol_bf16=1e-2, tol_f32=1e-4):
    if dtype == 'f16':
        _assert_f16(got, ref, name)
    else:
        assert_close(got, ref, tol_f32 if dtype == 'f32' else tol_bf16, name)


def _q_in(x, dtype):
    """Activations as the plan stores them."""
    return cnn_ref.bf16_round(x) if dtype == 'bf16' else cnn_ref.f16_round(x) if dtype == 'f16' else x


CONV_CASES = [
    # B, H, W, Cin, Cout, (kh,kw), stride, padding
    (2, 17, 15, 32, 32, (3, 3), 1, 'VALID'), (2, 17, 15, 32, 64, (3, 3), 1, 'SAME'),
    (2, 21, 21, 64, 80, (1, 1), 1, 'VALID'), (1, 19, 19, 80, 192, (3, 3), 1, 'VALID'),
    (2, 25, 25, 48, 64, (5, 5), 1, 'SAME'), (3, 25, 25, 288, 384, (3, 3), 2, 'VALID'),
    (2, 12, 12, 128, 128, (1, 7), 1, 'SAME'), (2, 12, 12, 160, 192, (7, 1), 1, 'SAME'),
    (2, 5, 5, 448, 384, (3, 3), 1, 'SAME'), (2, 5, 5, 384, 384, (1, 3), 1, 'SAME'),
    (2, 5, 5, 2048, 320, (1, 1), 1, 'SAME'), (70, 12, 12, 768, 192, (1, 1), 1, 'SAME'),
    (9, 25, 25, 192, 48, (1, 1), 1, 'SAME'), (1, 1, 1, 32, 16, (1, 1), 1, 'SAME')]


@pytest.mark.parametrize('dtype', ['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('case', CONV_CASES)
def test_conv_bn_relu(case, dtype):
    B, H, W, Cin, Cout, k, s, pad = case
    rng = np.random.default_rng(B * 1000 + H * 7 + Cin + Cout + k[0])
    x = rng.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((k[0], k[1], Cin, Cout)) / math.sqrt(k[0] * k[1] * Cin)).astype(np.float32)
    beta = 0.2 * rng.standard_normal(Cout).astype(np.float32)
    mean = 0.2 * rng.standard_normal(Cout).astype(np.float32)
    var = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    x = _q_in(x, dtype)
    ref = _ref_conv(x, w, beta, mean, var, s, pad, dtype)
    got = _run_conv(x, w, beta, mean, var, s, pad, dtype)
    # bf16: one output ulp (2^-8) on top of accumulation-order noise; f16: the fp32 bar against float64
    _check(got, ref, dtype, 'conv %s' % (case,))
    # concat slice: write at a channel offset of a wider buffer, neighbours untouched
    got2 = _run_conv(x, w, beta, mean, var, s, pad, dtype, dst_channels=Cout + 48, dst_coff=16)
    np.testing.assert_array_equal(got2[..., 16:16 + Cout], got)
    assert (got2[..., :16] == -7).all() and (got2[..., 16 + Cout:] == -7).all()


IM2COL_TILE_CASES = [CONV_CASES[i] for i in (1, 3, 5, 7, 8, 11, 12)]


@pytest.mark.parametrize('case', IM2COL_TILE_CASES)
def test_conv_im2col_tile_variants_identical_bits(case):
    _im2col_tile_variants(case, 'bf16')


@pytest.mark.parametrize('case', IM2COL_TILE_CASES)
def test_conv_im2col_tile_variants_identical_bits_f16(case):
    _im2col_tile_variants(case, 'f16')


def _im2col_tile_variants(case, dtype):
    """Every im2col LDS-DMA variant (ids 1..12: tile shapes x pipeline depths; 26..47: wide tiles (35..47 with loader waves), 4 or 8 waves) is a
    different blocking of the same sums in the same k order: bit-identical outputs, ragged row / channel tiles
    included, and correct against the oracle."""
    B, H, W, Cin, Cout, k, s, pad = case
    rng = np.random.default_rng(B * 1000 + H * 7 + Cin + Cout + k[0] + 5)
    x = _q_in(rng.standard_normal((B, H, W, Cin)).astype(np.float32), dtype)
    w = (rng.standard_normal((k[0], k[1], Cin, Cout)) / math.sqrt(k[0] * k[1] * Cin)).astype(np.float32)
    beta = 0.2 * rng.standard_normal(Cout).astype(np.float32)
    mean = 0.2 * rng.standard_normal(Cout).astype(np.float32)
    var = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    base = _run_conv(x, w, beta, mean, var, s, pad, dtype, tile=3)
    _check(base, _ref_conv(x, w, beta, mean, var, s, pad, dtype), dtype, 'conv %s' % (case,))
    for tile in list(range(1, 13)) + list(range(26, 48)):
        got = _run_conv(x, w, beta, mean, var, s, pad, dtype, tile=tile)
        np.testing.assert_array_equal(got, base, err_msg='tile %d %s' % (tile, case))


# patch-resident variants (tile ids 13..25, conv_patch.inc; 4, 8 and 12 waves per workgroup): stride 1, Cin >= 32.  The tile spans image
# boundaries (global output rows), ragged column tiles, SAME / VALID halos, the Kpad tail (K % 64 != 0),
# channel counts with and without the 32-byte pixel padding, Cout ragged against the channel tile.
PATCH_CASES = [
    # B, H, W, Cin, Cout, (kh,kw), padding
    (3, 17, 15, 32, 32, (3, 3), 'VALID'), (2, 37, 37, 32, 64, (3, 3), 'SAME'), (3, 19, 19, 80, 192, (3, 3), 'VALID'),
    (5, 25, 25, 48, 64, (5, 5), 'SAME'), (5, 25, 25, 96, 96, (3, 3), 'SAME'), (7, 12, 12, 128, 128, (1, 7), 'SAME'),
    (7, 12, 12, 160, 192, (7, 1), 'SAME'), (30, 5, 5, 448, 384, (3, 3), 'SAME'), (30, 5, 5, 384, 384, (1, 3), 'SAME'),
    (3, 21, 21, 64, 80, (1, 1), 'VALID'), (1, 1, 1, 32, 16, (1, 1), 'SAME'), (2, 40, 70, 32, 48, (3, 3), 'SAME')]


@pytest.mark.parametrize('tile', list(range(13, 26)) + list(range(48, 54)))
@pytest.mark.parametrize('case', PATCH_CASES)
def test_conv_patch_variants(case, tile):
    _patch_variant(case, tile, 'bf16')


@pytest.mark.parametrize('tile', list(range(13, 26)) + list(range(48, 54)))
@pytest.mark.parametrize('case', PATCH_CASES)
def test_conv_patch_variants_f16(case, tile):
    _patch_variant(case, tile, 'f16')


def _patch_variant(case, tile, dtype):
    B, H, W, Cin, Cout, k, pad = case
    rng = np.random.default_rng(B * 1000 + H * 7 + Cin + Cout + k[0] + tile)
    x = _q_in(rng.standard_normal((B, H, W, Cin)).astype(np.float32), dtype)
    w = (rng.standard_normal((k[0], k[1], Cin, Cout)) / math.sqrt(k[0] * k[1] * Cin)).astype(np.float32)
    beta = 0.2 * rng.standard_normal(Cout).astype(np.float32)
    mean = 0.2 * rng.standard_normal(Cout).astype(np.float32)
    var = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    ref = _ref_conv(x, w, beta, mean, var, 1, pad, dtype)
    try:
        got = _run_conv(x, w, beta, mean, var, 1, pad, dtype, tile=tile)
    except L.ComicHipError as e:
        assert 'not eligible' in str(e) and Cin >= 128      # the input window of a fat-Cin layer does not fit the LDS
        pytest.skip(str(e))
    _check(got, ref, dtype, 'patch conv %s tile %d' % (case, tile))
    # same operands and k order per accumulator as the im2col kernel: identical bits
    np.testing.assert_array_equal(got, _run_conv(x, w, beta, mean, var, 1, pad, dtype, tile=3))
    got2 = _run_conv(x, w, beta, mean, var, 1, pad, dtype, dst_channels=Cout + 48, dst_coff=16, tile=tile)
    np.testing.assert_array_equal(got2[..., 16:16 + Cout], got)
    assert (got2[..., :16] == -7).all() and (got2[..., 16 + Cout:] == -7).all()


def test_conv_patch_random_sweep():
    _patch_random_sweep('bf16')


def test_conv_patch_random_sweep_f16():
    _patch_random_sweep('f16')


def _patch_random_sweep(dtype):
    """Random stride-1 layer shapes, source / destination channel slices and batch sizes: every eligible
    patch-resident variant gives the bits of the im2col kernel (same operands, same k order); f16: the first cases'
    im2col results against float64 too."""
    tdt = _TDT[dtype]
    rng = np.random.default_rng(2024)
    n_ok = 0
    for case in range(40):
        kh, kw = [(1, 1), (3, 3), (5, 5), (1, 7), (7, 1), (1, 3), (3, 1), (3, 5)][rng.integers(8)]
        Cin = int(rng.choice([32, 48, 64, 80, 96, 112, 128, 160, 192]))
        Cout = int(rng.choice([16, 32, 48, 64, 80, 96, 128, 192, 208]))
        H, W, B = int(rng.integers(max(kh, 2), 40)), int(rng.integers(max(kw, 2), 40)), int(rng.integers(1, 9))
        pad = ['SAME', 'VALID'][rng.integers(2)]
        Ho, pt, _ = cnn_ref.out_size(H, kh, 1, pad)
        Wo, pl, _ = cnn_ref.out_size(W, kw, 1, pad)
        xc = Cin + int(rng.choice([0, 8, 64])); xo = int(rng.choice([0, 8])) if xc > Cin else 0
        yc = Cout + int(rng.choice([0, 16, 48])); yo = int(rng.choice([0, 4, 16])) if yc >= Cout + 16 else 0
        relu = int(rng.integers(2))
        x = torch.randn(B, H, W, xc, device=DEV).to(tdt)
        K = kh * kw * Cin
        wf = torch.randn(Cout, (K + 63) // 64 * 64, device=DEV) / K ** 0.5
        wf[:, K:] = 0
        w = wf.to(tdt).contiguous()
        scale, shift = torch.rand(Cout, device=DEV) + 0.5, torch.randn(Cout, device=DEV) * 0.1
        wt = L.ConvWeight(w.data_ptr(), scale.data_ptr(), shift.data_ptr())
        ref = None
        for tile in [3] + list(range(13, 26)) + list(range(48, 54)):
            y = torch.full((B, Ho, Wo, yc), -7.0, dtype=tdt, device=DEV)
            op = L.CnnOp(kind=0, src=0, dst=1, src_coff=xo, dst_coff=yo, H=H, W=W, Cin=Cin, Cout=Cout, KH=kh, KW=kw, SH=1,
                         SW=1, PT=pt, PL=pl, Ho=Ho, Wo=Wo, weight=0, relu=relu, out_f32=0, tile=tile)
            rc = lib().comic_conv2d_bn_relu(C.byref(op), x.data_ptr(), xc, y.data_ptr(), yc, C.byref(wt), B, _CODE[dtype],
                                            stream())
            sync()
            if rc != 0:
                assert tile != 3 and b'not eligible' in lib().comic_last_error()
                continue
            if tile == 3:
                ref = y
                if dtype == 'f16' and case < 6:     # the im2col kernel itself against float64 on the same operands
                    _assert_f16(y[..., yo:yo + Cout].float().cpu().numpy(),
                                _ref_from_packed(x[..., xo:xo + Cin], w, kh, kw, Cin, Cout, scale, shift, 1, pad, relu),
                                'sweep case %d' % case)
            else:
                assert torch.equal(y, ref), (case, tile, B, H, W, Cin, Cout, kh, kw, pad, xc, xo, yc, yo)
                n_ok += 1
    assert n_ok > 300


IMG_CASES = [   # (H, W, Cin, Cout, taps): every shape csrc/conv_img.hip is instantiated for
    (12, 12, 128, 192, (7, 1)), (12, 12, 128, 192, (1, 7)), (12, 12, 160, 192, (7, 1)), (12, 12, 192, 192, (1, 7)),
    (12, 12, 192, 192, (7, 1)), (12, 12, 128, 128, (1, 7)), (12, 12, 128, 128, (7, 1)), (12, 12, 160, 160, (1, 7)),
    (12, 12, 160, 160, (7, 1)), (25, 25, 64, 96, (3, 3)), (25, 25, 96, 96, (3, 3)), (5, 5, 448, 384, (3, 3)),
    (5, 5, 384, 384, (1, 3)), (5, 5, 384, 384, (3, 1))]


def _frag_weights(w, Cout, Kpad):
    """comic_cnn_pack_frag_weights on one [Cout][Kpad] 16-bit record."""
    out = torch.zeros_like(w)
    table = torch.tensor([[0, Cout, Kpad]], dtype=torch.int64, device=DEV)
    L.check(lib().comic_cnn_pack_frag_weights(w.data_ptr(), out.data_ptr(), table.data_ptr(), 1, w.numel(), stream()), 'pack')
    return out


def _ref_from_packed(x, w, kh, kw, Cin, Cout, scale, shift, stride, padding, relu):
    """float64 reference of a conv given as device tensors: 16-bit activations x [B][H][W][Cin], the packed filter
    w [Cout][Kpad] (k = (tap row, tap column, channel)), the folded fp32 scale / shift; output rounded once to f16."""
    K = kh * kw * Cin
    xs = x.double().cpu().numpy()
    ws = w.reshape(Cout, -1)[:, :K].double().cpu().numpy().reshape(Cout, kh, kw, Cin).transpose(1, 2, 3, 0)
    y = cnn_ref.conv2d(xs, ws, stride, padding) * scale.double().cpu().numpy() + shift.double().cpu().numpy()
    return cnn_ref.f16_round(np.maximum(y, 0) if relu else y)


@pytest.mark.parametrize('case', IMG_CASES)
def test_conv_image_resident_identical_bits(case):
    _image_resident(case, 'bf16')


@pytest.mark.parametrize('case', IMG_CASES)
def test_conv_image_resident_identical_bits_f16(case):
    _image_resident(case, 'f16')


def _image_resident(case, dtype):
    """The image-resident kernel (tile id 55: whole images in the LDS without halo, out-of-image taps read a zero page,
    weights streamed in fragment order) against the im2col kernel: same operands, same k order per accumulator ->
    identical bits.  Batch sizes that leave the last workgroup with fewer images than it has room for, source and
    destination channel slices, with and without ReLU; one launch with two members (a grouped launch's form) too.
    f16: the fragment-order pack of an f16 record, and the im2col result against float64 on the same operands."""
    H, W, Cin, Cout, (kh, kw) = case
    tdt, code = _TDT[dtype], _CODE[dtype]
    rng = np.random.default_rng(H * 131 + Cin + Cout + 7 * kh + kw)
    K = kh * kw * Cin
    Kpad = (K + 63) // 64 * 64
    pt, pl = (kh - 1) // 2, (kw - 1) // 2
    for B, xc, xo, yc, yo, relu in ((1, Cin, 0, Cout, 0, 1), (5, Cin + 64, 8, Cout + 48, 16, 1), (13, Cin, 0, Cout + 16, 4, 0)):
        x = torch.randn(B, H, W, xc, device=DEV).to(tdt)
        wf = torch.randn(Cout, Kpad, device=DEV) / K ** 0.5
        wf[:, K:] = 0
        w = wf.to(tdt).contiguous()
        frag = _frag_weights(w, Cout, Kpad)
        # the packing itself: lane l of step s of tile t holds W[16 t + (l & 15)][32 s + 8 (l >> 4) .. + 8]
        f = frag.view(Cout // 16, Kpad // 32, 64, 8)
        for t, s_, l in ((0, 0, 0), (Cout // 16 - 1, Kpad // 32 - 1, 63), (1, 3, 37)):
            assert torch.equal(f[t, s_, l].view(torch.int16),
                               w[16 * t + (l & 15), 32 * s_ + 8 * (l >> 4):32 * s_ + 8 * (l >> 4) + 8].view(torch.int16))
        scale, shift = torch.rand(Cout, device=DEV) + 0.5, torch.randn(Cout, device=DEV) * 0.1
        wt = L.ConvWeight(w.data_ptr(), scale.data_ptr(), shift.data_ptr(), frag.data_ptr())
        ys = {}
        for tile in (3, L.IMG_TILE):
            y = torch.full((B, H, W, yc), -7.0, dtype=tdt, device=DEV)
            op = L.CnnOp(kind=0, src=0, dst=1, src_coff=xo, dst_coff=yo, H=H, W=W, Cin=Cin, Cout=Cout, KH=kh, KW=kw, SH=1,
                         SW=1, PT=pt, PL=pl, Ho=H, Wo=W, weight=0, relu=relu, out_f32=0, tile=tile)
            L.check(lib().comic_conv2d_bn_relu(C.byref(op), x.data_ptr(), xc, y.data_ptr(), yc, C.byref(wt), B, code, stream()),
                    'conv tile %d' % tile)
            sync()
            ys[tile] = y
        assert torch.equal(ys[L.IMG_TILE].view(torch.int16), ys[3].view(torch.int16)), (case, B)
        assert bool((ys[3][..., yo:yo + Cout].float().abs().max() > 0.1))
        if dtype == 'f16' and B < 13:
            _assert_f16(ys[L.IMG_TILE][..., yo:yo + Cout].float().cpu().numpy(),
                        _ref_from_packed(x[..., xo:xo + Cin], w, kh, kw, Cin, Cout, scale, shift, 1, 'SAME', relu),
                        'image-resident %s B=%d' % (case, B))
    # without fragment-order weights the id is refused, like a patch id on an ineligible layer
    wt0 = L.ConvWeight(w.data_ptr(), scale.data_ptr(), shift.data_ptr())
    op = L.CnnOp(kind=0, src=0, dst=1, H=H, W=W, Cin=Cin, Cout=Cout, KH=kh, KW=kw, SH=1, SW=1, PT=pt, PL=pl, Ho=H, Wo=W,
                 weight=0, relu=1, tile=L.IMG_TILE)
    assert lib().comic_conv2d_bn_relu(C.byref(op), x.data_ptr(), xc, y.data_ptr(), yc, C.byref(wt0), B, code, stream()) != 0
    assert b'not eligible' in lib().comic_last_error()


def test_conv_patch_rejects_strided():
    x = np.zeros((1, 9, 9, 32), np.float32)
    w = np.zeros((3, 3, 32, 32), np.float32)
    z, o = np.zeros(32, np.float32), np.ones(32, np.float32)
    with pytest.raises(L.ComicHipError):
        _run_conv(x, w, z, z, o, 2, 'VALID', 'bf16', tile=13)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_stem_conv(dtype):
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (2, 37, 41, 3)).astype(np.float32)
    w = (rng.standard_normal((3, 3, 3, 32)) / 5).astype(np.float32)
    beta = 0.1 * rng.standard_normal(32).astype(np.float32)
    mean = 0.1 * rng.standard_normal(32).astype(np.float32)
    var = rng.uniform(0.5, 1.5, 32).astype(np.float32)
    # the stem reads fp32 images and fp32 weights in both modes; only the store is bf16
    ref = cnn_ref.batch_norm_inference(cnn_ref.conv2d(x, w, 2, 'VALID'), beta, mean, var)
    ref = np.maximum(ref, 0)
    got = _run_conv(x, w, beta, mean, var, 2, 'VALID', dtype)
    assert_close(got, cnn_ref.bf16_round(ref) if dtype == 'bf16' else ref, 1e-4 if dtype == 'f32' else 5e-3, 'stem')


# the three stem kernels: the 3x3x3 VALID MFMA form (Inception-V3 Conv2d_1a), the direct kernel (tile 1), and
# conv_stem_wide_kernel at Inception-V1's Conv2d_1a_7x7 shape (7x7 / 2 SAME, 3 -> 64; 16-bit plans only)
STEM_CASES = [((2, 37, 41, 3), (3, 3), 32, 2, 'VALID', 0), ((2, 37, 41, 3), (3, 3), 32, 2, 'VALID', 1),
              ((1, 224, 224, 3), (7, 7), 64, 2, 'SAME', 0), ((2, 30, 36, 3), (7, 7), 64, 2, 'SAME', 1)]


@pytest.mark.parametrize('case', STEM_CASES)
def test_stem_conv_f16(case):
    """f16 plans: the stem reads the fp32 image and fp32 filter, accumulates in fp32 and stores f16 once -- against
    float64 with one rounding of the output, at the fp32 bar; the three stem kernels give the bits of each other where
    two of them take the same layer."""
    shape, (kh, kw), Cout, s, pad, tile = case
    rng = np.random.default_rng(sum(shape) + Cout)
    x = rng.uniform(-1, 1, shape).astype(np.float32)
    w = (rng.standard_normal((kh, kw, 3, Cout)) / math.sqrt(kh * kw * 3)).astype(np.float32)
    beta = 0.1 * rng.standard_normal(Cout).astype(np.float32)
    mean = 0.1 * rng.standard_normal(Cout).astype(np.float32)
    var = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    got = _run_conv(x, w, beta, mean, var, s, pad, 'f16', tile=tile)
    _assert_f16(got, _ref_conv(x, w, beta, mean, var, s, pad, 'f16'), 'stem %s tile %d' % (shape, tile))
    if tile == 0:       # the direct kernel on the same layer: the same products in another order, within the bar
        _assert_f16(_run_conv(x, w, beta, mean, var, s, pad, 'f16', tile=1), _ref_conv(x, w, beta, mean, var, s, pad, 'f16'),
                    'stem direct %s' % (shape,))


def _run_pool(x, kind, k, s, pad, dtype, dst_channels=None, dst_coff=0, tile=0):
    B, H, W, Cc = x.shape
    kh, kw = (k, k) if isinstance(k, int) else k
    Ho, pt, _ = cnn_ref.out_size(H, kh, s, pad)
    Wo, pl, _ = cnn_ref.out_size(W, kw, s, pad)
    tdt = _TDT[dtype]
    xd = dev(x).to(tdt)
    yc = dst_channels or Cc
    y = torch.full((B, Ho, Wo, yc), -7.0, dtype=torch.float32 if kind == 4 else tdt, device=DEV)
    op = L.CnnOp(kind=kind, src=0, dst=1, src_coff=0, dst_coff=dst_coff, H=H, W=W, Cin=Cc, Cout=Cc, KH=kh, KW=kw,
                 SH=s, SW=s, PT=pt, PL=pl, Ho=Ho, Wo=Wo, weight=-1, relu=0, out_f32=int(kind == 4), tile=tile)
    L.check(lib().comic_conv2d_bn_relu(C.byref(op), xd.data_ptr(), Cc, y.data_ptr(), yc, None, B,
                                       _CODE[dtype], stream()), 'pool')
    sync()
    return y.float().cpu().numpy()


def _run_pool_bn_relu(x, beta, mean, var, dtype, tile, relu=1, out_f32=0, dst_channels=None, dst_coff=0):
    """Kind 7: 3x3 / 1 SAME average of an fp32 map (the raw 1x1 projection of a pool branch), then the folded BatchNorm
    and ReLU, stored in the plan's 16-bit format (or fp32 with out_f32).  tile 1: the row-walking kernel
    (pool_bn_relu_rows_kernel), tile 2: one thread per pixel (pool_bn_relu_kernel)."""
    B, H, W, Cc = x.shape
    scale = torch.empty(Cc, device=DEV); shift = torch.empty(Cc, device=DEV)
    L.check(lib().comic_fold_bn(P(beta), P(mean), P(var), 1e-3, scale.data_ptr(), shift.data_ptr(), Cc, stream()))
    xd = dev(x)
    yc = dst_channels or Cc
    y = torch.full((B, H, W, yc), -7.0, dtype=torch.float32 if out_f32 else _TDT[dtype], device=DEV)
    op = L.CnnOp(kind=7, src=0, dst=1, src_coff=0, dst_coff=dst_coff, H=H, W=W, Cin=Cc, Cout=Cc, KH=3, KW=3, SH=1, SW=1,
                 PT=1, PL=1, Ho=H, Wo=W, weight=0, relu=relu, out_f32=out_f32, src_f32=1, tile=tile)
    wt = L.ConvWeight(None, scale.data_ptr(), shift.data_ptr())
    L.check(lib().comic_conv2d_bn_relu(C.byref(op), xd.data_ptr(), Cc, y.data_ptr(), yc, C.byref(wt), B, _CODE[dtype],
                                       stream()), 'pool+bn')
    sync()
    return y


def test_device_image_preprocess_matches_numpy_pipeline():
    """comic_image_preprocess (uint8 -> [0,1] -> TF-1 bilinear 256x256 -> flip -> crop -> [-1,1]) against the ORACLE's
    restatement of inception_preprocessing_radix.py:158-278 (oracle/preprocess_ref.py), bit for bit: odd sizes, up- and
    down-scaling, flips, crop offsets; staging slots re-used across calls; and the product's own host path against it."""
    from comic_amd import inputs
    from oracle import preprocess_ref
    rng = np.random.default_rng(5)
    pre = inputs.DevicePreprocessor(DEV, 224, 224)
    for rep in range(3):
        sizes = [(480, 640), (333, 500), (100, 77), (256, 256), (1, 1), (257, 1023)][:6 - rep]
        ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
        params = [(bool(rng.integers(2)), int(rng.integers(0, 33)), int(rng.integers(0, 33))) for _ in ims]
        got = pre(ims, params).cpu().numpy()
        for i, (im, prm) in enumerate(zip(ims, params)):
            want = preprocess_ref.preprocess_image(im, 224, 224, *prm)
            np.testing.assert_array_equal(got[i], want, err_msg='image %d %s %s' % (i, im.shape, prm))
            np.testing.assert_array_equal(inputs.preprocess_image(im, 224, 224, True, None, prm), want)
    pre299 = inputs.DevicePreprocessor(DEV, 256, 256)          # no crop margin
    im = rng.integers(0, 256, (300, 300, 3), dtype=np.uint8)
    np.testing.assert_array_equal(pre299([im], [(True, 0, 0)]).cpu().numpy()[0],
                                  preprocess_ref.preprocess_image(im, 256, 256, True, 0, 0))


@pytest.mark.parametrize('dtype', ['f32', 'bf16', 'f16'])
def test_pools(dtype):
    rng = np.random.default_rng(1)
    x = _q_in(rng.standard_normal((3, 13, 11, 64)).astype(np.float32), dtype)
    np.testing.assert_array_equal(_run_pool(x, 2, 3, 2, 'VALID', dtype), cnn_ref.max_pool(x, 3, 2, 'VALID'))
    got = _run_pool(x, 3, 3, 1, 'SAME', dtype)
    if dtype == 'f16':          # fp32 sum / count, one RNE store: against float64
        _assert_f16(got, cnn_ref.f16_round(cnn_ref.avg_pool(x.astype(np.float64), 3, 1, 'SAME')), 'avgpool')
    else:
        q = cnn_ref.bf16_round if dtype == 'bf16' else (lambda a: a)
        assert_close(got, q(cnn_ref.avg_pool(x, 3, 1, 'SAME')), 1e-6 if dtype == 'f32' else 5e-3, 'avgpool')
    got = _run_pool(x, 2, 3, 2, 'VALID', dtype, dst_channels=160, dst_coff=96)
    np.testing.assert_array_equal(got[..., 96:], cnn_ref.max_pool(x, 3, 2, 'VALID'))
    x5 = x[:, :5, :5, :]
    got = _run_pool(x5, 4, 5, 1, 'VALID', dtype)
    assert_close(got, cnn_ref.avg_pool(x5, 5, 1, 'VALID'), 1e-5, 'global avgpool')
    got = _run_pool(x[:, :9, :9, :], 4, 8, 1, 'VALID', dtype)        # 9x9 map, 8x8 window -> 2x2
    assert_close(got, cnn_ref.avg_pool(x[:, :9, :9, :], 8, 1, 'VALID'), 1e-5, 'global avgpool 8x8')
    if dtype != 'f32':
        # the stride-1 3x3 SAME max-pool of Inception-V1: the row-walking kernel (tile 1) and the per-pixel one (tile 2)
        want = cnn_ref.max_pool(x, 3, 1, 'SAME')
        for tile in (1, 2):
            np.testing.assert_array_equal(_run_pool(x, 2, 3, 1, 'SAME', dtype, tile=tile), want, err_msg='tile %d' % tile)


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('shape', [(3, 13, 11, 64), (2, 25, 25, 96), (1, 5, 5, 32)])
def test_pool_bn_relu(shape, dtype):
    """Kind 7 on both kernels (row walk and per pixel): against float64 (average, BatchNorm, ReLU) with one rounding of
    the output -- f16 at the fp32 bar, bf16 within one output ulp; the two kernels sum in different orders, so they
    are each held to the reference; a destination channel slice leaves its neighbours untouched."""
    B, H, W, Cc = shape
    rng = np.random.default_rng(B * H + Cc)
    x = (2 * rng.standard_normal(shape)).astype(np.float32)
    beta = 0.2 * rng.standard_normal(Cc).astype(np.float32)
    mean = 0.2 * rng.standard_normal(Cc).astype(np.float32)
    var = rng.uniform(0.5, 1.5, Cc).astype(np.float32)
    scale = 1.0 / np.sqrt(var.astype(np.float64) + cnn_ref.BN_EPS)
    for relu in (1, 0):
        y = cnn_ref.avg_pool(x.astype(np.float64), 3, 1, 'SAME')
        y = (y - mean) * scale + beta
        y = np.maximum(y, 0) if relu else y
        for tile in (1, 2):
            got = _run_pool_bn_relu(x, beta, mean, var, dtype, tile, relu=relu).float().cpu().numpy()
            if dtype == 'f16':
                _assert_f16(got, cnn_ref.f16_round(y), 'pool+bn %s tile %d' % (shape, tile))
            else:
                assert_close(got, cnn_ref.bf16_round(y.astype(np.float32)), 1e-2, 'pool+bn %s tile %d' % (shape, tile))
    got = _run_pool_bn_relu(x, beta, mean, var, dtype, 1, dst_channels=Cc + 24, dst_coff=8).float().cpu().numpy()
    assert (got[..., :8] == -7).all() and (got[..., 8 + Cc:] == -7).all()
    np.testing.assert_array_equal(got[..., 8:8 + Cc], _run_pool_bn_relu(x, beta, mean, var, dtype, 1).float().cpu().numpy())


@pytest.mark.parametrize('case', [(3, 25, 25, 288, 64, 0), (2, 25, 25, 192, 48, 0), (2, 21, 19, 64, 80, 0),
                                  (3, 23, 23, 64, 80, L.OP_POOLED_SRC), (2, 13, 12, 192, 48, L.OP_POOLED_SRC),
                                  (1, 13, 13, 192, 256, L.OP_POOLED_SRC)])
def test_conv_weight_stationary_f16(case):
    """Single 1x1 convs on the weight-stationary kernel (tile id 54, csrc/conv_ws.hip) on f16, plain and with
    COMIC_OP_POOLED_SRC (the 3x3 / 2 VALID max-pool folded into the loads): against max-pool-then-conv in float64 at the
    fp32 bar, and bit for bit against the im2col kernel on the same (pooled) operands."""
    B, H, W, Cin, Cout, flags = case
    rng = np.random.default_rng(B + H + W + Cin + Cout + flags)
    x = cnn_ref.f16_round(rng.standard_normal((B, H, W, Cin)).astype(np.float32))
    w = (rng.standard_normal((1, 1, Cin, Cout)) / math.sqrt(Cin)).astype(np.float32)
    beta = 0.2 * rng.standard_normal(Cout).astype(np.float32)
    mean = 0.2 * rng.standard_normal(Cout).astype(np.float32)
    var = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    xin = cnn_ref.max_pool(x, 3, 2, 'VALID') if flags else x          # exact in f16
    ref = _ref_conv(xin, w, beta, mean, var, 1, 'SAME', 'f16')
    got = _run_conv(x, w, beta, mean, var, 1, 'SAME', 'f16', tile=L.WS_TILE, flags=flags)
    _assert_f16(got, ref, 'ws %s' % (case,))
    np.testing.assert_array_equal(got, _run_conv(xin, w, beta, mean, var, 1, 'SAME', 'f16', tile=3))
    got2 = _run_conv(x, w, beta, mean, var, 1, 'SAME', 'f16', tile=L.WS_TILE, flags=flags, dst_channels=Cout + 32, dst_coff=16)
    np.testing.assert_array_equal(got2[..., 16:16 + Cout], got)
    assert (got2[..., :16] == -7).all() and (got2[..., 16 + Cout:] == -7).all()


# ---- the 16-bit store is IEEE conversion (RNE, subnormals, overflow to inf) ------------------------------------------
def _range_bn(Cout, dtype):
    """Per-channel (beta, mean, var) putting the outputs of a conv with O(1) products in four ranges (a quarter of the
    channels each): f16 subnormals (scale 2^-19), around 1, just below 65504 (shift 65490) and past 65520 (shift 7e4).
    relu is off, so each range holds both signs where the shift does not dominate."""
    q = Cout // 4
    scale = np.concatenate([np.full(q, 2.0 ** -19), np.ones(q), np.full(q, 4.0), np.ones(Cout - 3 * q)])
    shift = np.concatenate([np.zeros(q), np.zeros(q), np.full(q, 65490.0), np.full(Cout - 3 * q, 7e4)])
    var = (1.0 / scale ** 2 - cnn_ref.BN_EPS).astype(np.float32)
    mean = np.zeros(Cout, np.float32)
    return shift.astype(np.float32), mean, var


def _store_cases():
    # (name, B, H, W, Cin, Cout, (kh, kw), stride, padding, tile, flags)
    return [('im2col', 2, 9, 9, 64, 64, (3, 3), 1, 'SAME', 3, 0), ('im2col wide', 2, 9, 9, 64, 64, (3, 3), 1, 'SAME', 26, 0),
            ('patch', 2, 9, 9, 64, 64, (3, 3), 1, 'SAME', 13, 0), ('patch loader waves', 2, 9, 9, 64, 64, (3, 3), 1, 'SAME', 48, 0),
            ('image-resident', 3, 12, 12, 128, 128, (1, 7), 1, 'SAME', L.IMG_TILE, 0),
            ('weight-stationary', 2, 9, 9, 64, 64, (1, 1), 1, 'SAME', L.WS_TILE, 0),
            ('weight-stationary pooled', 2, 11, 11, 64, 64, (1, 1), 1, 'SAME', L.WS_TILE, L.OP_POOLED_SRC),
            ('stem mfma', 2, 17, 19, 3, 32, (3, 3), 2, 'VALID', 0, 0), ('stem direct', 2, 17, 19, 3, 32, (3, 3), 2, 'VALID', 1, 0),
            ('stem wide', 1, 224, 224, 3, 64, (7, 7), 2, 'SAME', 0, 0)]


def _conv_f32_and_16(case, dtype, x, w, beta, mean, var):
    name, B, H, W, Cin, Cout, (kh, kw), s, pad, tile, flags = case
    if tile == L.IMG_TILE:          # fragment-order weights: through the device-tensor path
        K = kh * kw * Cin
        Kpad = (K + 63) // 64 * 64
        tdt, code = _TDT[dtype], _CODE[dtype]
        wd = dev(w)
        packed = torch.zeros(Cout * Kpad, dtype=tdt, device=DEV)
        L.check(lib().comic_pack_conv_weights(wd.data_ptr(), packed.data_ptr(), kh, kw, Cin, Cout, code, stream()))
        frag = _frag_weights(packed, Cout, Kpad)
        scale = torch.empty(Cout, device=DEV); shift = torch.empty(Cout, device=DEV)
        L.check(lib().comic_fold_bn(P(beta), P(mean), P(var), 1e-3, scale.data_ptr(), shift.data_ptr(), Cout, stream()))
        wt = L.ConvWeight(packed.data_ptr(), scale.data_ptr(), shift.data_ptr(), frag.data_ptr())
        xd = dev(x).to(tdt)
        outs = []
        for out_f32 in (1, 0):
            y = torch.full((B, H, W, Cout), -7.0, dtype=torch.float32 if out_f32 else tdt, device=DEV)
            op = L.CnnOp(kind=0, src=0, dst=1, H=H, W=W, Cin=Cin, Cout=Cout, KH=kh, KW=kw, SH=1, SW=1, PT=(kh - 1) // 2,
                         PL=(kw - 1) // 2, Ho=H, Wo=W, weight=0, relu=0, out_f32=out_f32, tile=tile)
            L.check(lib().comic_conv2d_bn_relu(C.byref(op), xd.data_ptr(), Cin, y.data_ptr(), Cout, C.byref(wt), B, code,
                                               stream()), name)
            sync()
            outs.append(y)
        return outs
    return [torch.from_numpy(_run_conv(x, w, beta, mean, var, s, pad, dtype, relu=0, out_f32=o, tile=tile, flags=flags))
            for o in (1, 0)]


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('case', _store_cases(), ids=lambda c: c[0].replace(' ', '_'))
def test_conv_16bit_store_is_ieee_conversion(case, dtype):
    """The same launch with out_f32 = 1 and with the 16-bit store: the work is the same, so the 16-bit output must be the
    IEEE conversion of the fp32 one bit for bit -- RNE, subnormal outputs kept, overflow past 65520 to +-inf (what torch
    does) -- over outputs in the f16 subnormal range, around 1, just below 65504 and past 65520."""
    name, B, H, W, Cin, Cout, (kh, kw), s, pad, tile, flags = case
    rng = np.random.default_rng(Cin * 7 + Cout + kh)
    x = _q_in(rng.standard_normal((B, H, W, Cin)).astype(np.float32), dtype) if Cin > 4 else \
        rng.uniform(-1, 1, (B, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((kh, kw, Cin, Cout)) * (8.0 / math.sqrt(kh * kw * Cin))).astype(np.float32)
    beta, mean, var = _range_bn(Cout, dtype)
    y32, y16 = _conv_f32_and_16(case, dtype, x, w, beta, mean, var)
    y32 = torch.as_tensor(y32).float().cpu()
    want = y32.half() if dtype == 'f16' else y32.bfloat16()
    got = torch.as_tensor(y16).cpu().to(want.dtype)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
        '%s: %d of %d values differ' % (name, int((got.view(torch.int16) != want.view(torch.int16)).sum()), got.numel())
    if dtype == 'f16':          # the four ranges were all reached
        a = y32.abs()
        q = Cout // 4
        assert ((a[..., :q] < 2.0 ** -14) & (a[..., :q] > 0)).float().mean() > 0.5
        assert (want[..., 2 * q:3 * q].float() == 65504).any() and torch.isinf(want[..., 3 * q:].float()).all()
        assert (want[..., 2 * q:3 * q].float() < 65504).any()


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('tile', [1, 2])
def test_pool_bn_relu_16bit_store_is_ieee_conversion(tile, dtype):
    """Kind 7's 16-bit store against its own fp32 store, bit for bit, over the four output ranges."""
    rng = np.random.default_rng(tile)
    x = (8 * rng.standard_normal((2, 9, 11, 64))).astype(np.float32)
    beta, mean, var = _range_bn(64, dtype)
    y32 = _run_pool_bn_relu(x, beta, mean, var, dtype, tile, relu=0, out_f32=1).cpu()
    y16 = _run_pool_bn_relu(x, beta, mean, var, dtype, tile, relu=0).cpu()
    want = y32.half() if dtype == 'f16' else y32.bfloat16()
    assert torch.equal(y16.view(torch.int16), want.view(torch.int16))


def _f16_edge_vector():
    from tests.test_oracle_cnn import F16_EDGES
    rng = np.random.default_rng(0)
    rand = np.concatenate([rng.standard_normal(4000), rng.standard_normal(2000) * 2.0 ** -17,
                           rng.uniform(3e4, 7e4, 2000)])
    # fp32 values on both sides of every f16 rounding boundary near the edges
    mids = np.array([(2 * k + 1) * 2.0 ** -25 for k in range(8)] + [1 + 2.0 ** -11, 65504 + 8, 65504 + 16])
    near = np.concatenate([np.nextafter(mids.astype(np.float32), np.float32(np.inf)),
                           np.nextafter(mids.astype(np.float32), np.float32(-np.inf)), mids])
    v = np.concatenate([F16_EDGES, -F16_EDGES, rand, -rand, near, -near]).astype(np.float32)
    return np.concatenate([v, np.zeros(-len(v) % 64, np.float32)])


def test_f16_weight_conversion_is_ieee():
    """The two routes by which weights reach f16 -- comic_cnn_refresh_weights_dtype (the product's plan copy) and
    comic_pack_conv_weights (code 2) -- against master.half(), bit for bit, over the edge classes of IEEE half."""
    v = _f16_edge_vector()
    n = v.size
    master = dev(v)
    want = master.cpu().half()
    cout = 64
    out = torch.zeros(n, dtype=torch.float16, device=DEV)
    beta = torch.zeros(cout, device=DEV); mean = torch.zeros(cout, device=DEV)
    scale = torch.ones(cout, device=DEV); shift = torch.empty(cout, device=DEV)
    L.check(lib().comic_cnn_refresh_weights_dtype(master.data_ptr(), out.data_ptr(), n, beta.data_ptr(), mean.data_ptr(),
                                                  scale.data_ptr(), shift.data_ptr(), cout, 2, stream()), 'refresh')
    sync()
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16)), \
        'refresh: %d values differ' % int((out.cpu().view(torch.int16) != want.view(torch.int16)).sum())
    # pack: HWIO [1][1][K][Cout] -> [Cout][Kpad], padding columns zero
    K = n // cout
    Kpad = (K + 63) // 64 * 64
    packed = torch.full((cout, Kpad), 7.0, dtype=torch.float16, device=DEV)
    L.check(lib().comic_pack_conv_weights(master.data_ptr(), packed.data_ptr(), 1, 1, K, cout, 2, stream()), 'pack')
    sync()
    wantp = want.reshape(K, cout).t().contiguous()
    assert torch.equal(packed[:, :K].cpu().view(torch.int16), wantp.view(torch.int16))
    assert not packed[:, K:].view(torch.int16).any()


@pytest.mark.parametrize('which', ['inputs', 'weights'])
def test_conv_f16_subnormal_operands(which):
    """f16 operands in the subnormal range (|v| in [2^-24, 2^-14)) on the MFMA path: subnormal activations with weights
    large enough that the products are normal, then the reverse -- against float64 on the same operands at the fp32 bar.
    This measures whether v_mfma_f32_16x16x32_f16 on gfx950 keeps f16 subnormal A / B operands: it does (a flush would put
    the result at the BatchNorm shift alone)."""
    rng = np.random.default_rng(3 if which == 'inputs' else 4)
    B, H, W, Cin, Cout = 2, 9, 9, 64, 64
    sub = lambda shape: (np.sign(rng.standard_normal(shape)) * rng.uniform(2.0 ** -24, 2.0 ** -14, shape)).astype(np.float32)
    if which == 'inputs':
        x = cnn_ref.f16_round(sub((B, H, W, Cin)))
        w = (rng.standard_normal((3, 3, Cin, Cout)) * 2.0 ** 12).astype(np.float32)
    else:
        x = cnn_ref.f16_round(rng.standard_normal((B, H, W, Cin)).astype(np.float32))
        w = sub((3, 3, Cin, Cout))
    x16 = cnn_ref.f16_round(x); w16 = cnn_ref.f16_round(w)
    sub_share = np.mean((np.abs(x16 if which == 'inputs' else w16) < 2.0 ** -14) & ((x16 if which == 'inputs' else w16) != 0))
    assert sub_share > 0.95
    # scale the products back to O(1) through the BatchNorm (subnormal weights: var small)
    ref_raw = cnn_ref.conv2d(x16.astype(np.float64), w16.astype(np.float64), 1, 'SAME')
    amp = float(np.abs(ref_raw).max())
    var = np.full(Cout, max((amp / 4.0) ** 2 - cnn_ref.BN_EPS, 0.0), np.float32)
    beta = np.zeros(Cout, np.float32); mean = np.zeros(Cout, np.float32)
    ref = _ref_conv(x16, w16, beta, mean, var, 1, 'SAME', 'f16', relu=0)
    for tile in (3, 13, 26):
        got = _run_conv(x16, w16, beta, mean, var, 1, 'SAME', 'f16', relu=0, tile=tile)
        _assert_f16(got, ref, 'subnormal %s tile %d' % (which, tile))


# ------------------------------------------------------------------------ decoder kernels --
def test_embed_fwd_bwd():
    rng = np.random.default_rng(2)
    V, E, rows = 258, 256, 150
    table = rng.standard_normal((V, E)).astype(np.float32)
    ids = rng.integers(-1, V, rows).astype(np.int32)
    out = torch.empty((rows, E), device=DEV)
    L.check(lib().comic_embed_fwd(P(table), P(ids), out.data_ptr(), rows, E, V, stream()))
    np.testing.assert_array_equal(out.cpu().numpy(), dr.embed(table, ids))
    dout = rng.standard_normal((rows, E)).astype(np.float32)
    dt = torch.zeros((V, E), device=DEV)
    L.check(lib().comic_embed_bwd(P(ids), P(dout), dt.data_ptr(), rows, E, V, stream()))
    ref = np.zeros((V, E), np.float64)
    np.add.at(ref, ids[ids >= 0], dout[ids >= 0])
    assert_close(dt.cpu().numpy(), ref, 1e-6, 'embed_bwd')


@pytest.mark.parametrize('V,E,rows,hot', [(258, 256, 6048, 4800),      # a 224-hypothesis SCST step of long captions: radix digit 0 on 80 %
                                          (258, 256, 9000, 9000),      # one id on every row: the LDS list (4096 entries) runs full twice
                                          (40, 100, 5000, 4500),       # E % 64 != 0: a partly used column slice
                                          (3000, 64, 2000, 1500),      # many vocabulary rows: still the 1024-thread form (V * slices <= 4096)
                                          (25599, 256, 1280, 300),     # word vocabulary: the one-wave-per-stream form
                                          (300, 30, 5000, 4700)])      # E % 4 != 0: scalar columns
def test_embed_bwd_skewed_ids_and_list_overflow(V, E, rows, hot):
    """comic_embed_bwd on frequency-skewed ids (the reference vocabulary is frequency-sorted, prepro_base.py:186: one radix digit
    sits on most tokens): `hot` rows carry id 1 -- more than the kernel's LDS list holds in two of the cases, so the
    flush-and-refill path runs -- the rest are uniform with PAD (-1) among them.  Accumulating form (+=) against a float64
    scatter-add; two runs give the same bits."""
    rng = np.random.default_rng(V + rows)
    ids = rng.integers(-1, V, rows).astype(np.int32)
    ids[rng.permutation(rows)[:hot]] = 1
    dout = rng.standard_normal((rows, E)).astype(np.float32)
    base = rng.standard_normal((V, E)).astype(np.float32)
    d_ids, d_dout = dev(ids), dev(dout)
    runs = []
    for _ in range(2):
        dt = dev(base)
        L.check(lib().comic_embed_bwd(d_ids.data_ptr(), d_dout.data_ptr(), dt.data_ptr(), rows, E, V, stream()))
        runs.append(dt.cpu().numpy())
    ref = base.astype(np.float64)
    np.add.at(ref, ids[ids >= 0], dout[ids >= 0].astype(np.float64))
    assert_close(runs[0], ref, 2e-6, 'embed_bwd skewed')
    np.testing.assert_array_equal(runs[0], runs[1])
    untouched = np.setdiff1d(np.arange(V), ids[ids >= 0])
    np.testing.assert_array_equal(runs[0][untouched], base[untouched])


def test_dropout_mask_and_apply():
    n = 1 << 20
    m = torch.empty(n, device=DEV)
    L.check(lib().comic_dropout_mask(m.data_ptr(), n, 0.65, 1234, 0, stream()))
    m2 = torch.empty(n, device=DEV)
    L.check(lib().comic_dropout_mask(m2.data_ptr(), n, 0.65, 1234, 0, stream()))
    m3 = torch.empty(n, device=DEV)
    L.check(lib().comic_dropout_mask(m3.data_ptr(), n, 0.65, 1235, 0, stream()))
    mm = m.cpu().numpy()
    assert set(np.unique(mm)) <= {0.0, 1.0}
    assert abs(mm.mean() - 0.65) < 3e-3
    assert torch.equal(m, m2) and not torch.equal(m, m3)
    x = torch.randn(n, device=DEV)
    y = torch.empty_like(x)
    L.check(lib().comic_dropout_apply(x.data_ptr(), m.data_ptr(), 0.65, y.data_ptr(), n, stream()))
    np.testing.assert_array_equal(y.cpu().numpy(), (x.cpu().numpy() / np.float32(0.65)) * mm)


def test_dropout_masks4_equals_four_calls():
    """comic_dropout_masks4_dev (the four masks of a training step in one launch, keep probability per segment) gives
    the bits of four comic_dropout_mask calls with cumulative counter offsets."""
    n4 = [1000, 70001, 33333, 257]
    keep4 = [0.65, 0.65, 0.5, 0.9]
    seed = 0x9E3779B9 + 5
    buf = torch.empty(sum(n4), device=DEV)
    seed_dev = torch.tensor([seed], dtype=torch.int64, device=DEV)
    L.check(lib().comic_dropout_masks4_dev(buf.data_ptr(), (C.c_int64 * 4)(*n4), (C.c_float * 4)(*keep4),
                                           seed_dev.data_ptr(), stream()))
    off = 0
    for n, keep in zip(n4, keep4):
        m = torch.empty(n, device=DEV)
        L.check(lib().comic_dropout_mask(m.data_ptr(), n, keep, seed, off, stream()))
        assert torch.equal(m, buf[off:off + n]), (n, keep)
        off += n


def test_lstm_gates_fwd_bwd():
    rng = np.random.default_rng(3)
    B, D = 6, 128
    g = rng.standard_normal((B, 4 * D)).astype(np.float32)
    c = rng.standard_normal((B, D)).astype(np.float32)
    h = rng.standard_normal((B, D)).astype(np.float32)
    mask = (rng.random((B, D)) < 0.65).astype(np.float32)
    lens = np.array([3, 1, 5, 2, 9, 2], np.int32)
    t = 2
    fin = t >= lens
    i, j, f, o = g[:, :D], g[:, D:2 * D], g[:, 2 * D:3 * D], g[:, 3 * D:]
    si, tj, sf, so = dr.sigmoid(i), np.tanh(j), dr.sigmoid(f + 1), dr.sigmoid(o)
    c2 = c * sf + si * tj
    tc = np.tanh(c2)
    h2 = tc * so
    y = h2 / np.float32(0.65) * mask
    outs = {k: torch.empty((B, D), device=DEV) for k in ('c_new', 'h_new', 'y', 'cs', 'hs')}
    ga = torch.empty((B, 4 * D), device=DEV)
    L.check(lib().comic_lstm_gates_fwd(P(g), P(c), P(h), ga.data_ptr(),
                                       outs['c_new'].data_ptr(), outs['h_new'].data_ptr(), outs['y'].data_ptr(),
                                       P(mask), 0.65, P(lens), t, outs['cs'].data_ptr(),
                                       outs['hs'].data_ptr(), B, D, stream()))
    assert_close(outs['c_new'].cpu().numpy(), c2, 1e-5, 'c_new')
    assert_close(outs['y'].cpu().numpy(), y, 1e-5, 'y')
    assert_close(outs['cs'].cpu().numpy(), np.where(fin[:, None], c, c2), 1e-5, 'c_state')
    assert_close(outs['hs'].cpu().numpy(), np.where(fin[:, None], h, h2), 1e-5, 'h_state')
    assert_close(ga.cpu().numpy(), np.concatenate([si, tj, sf, so], 1), 1e-5, 'gates')
    # backward vs the oracle's cell backward
    dc = rng.standard_normal((B, D)).astype(np.float32)
    dh = rng.standard_normal((B, D)).astype(np.float32)
    dy = rng.standard_normal((B, D)).astype(np.float32)
    live = (~fin)[:, None].astype(np.float32)
    dh2 = dh * live + dy / np.float32(0.65) * mask
    dg_ref, dcp_ref = dr._lstm_backward(None, (si, tj, sf, so, tc), c, dc * live, dh2, D)
    d_dc, d_dh = dev(dc), dev(dh)
    dg = torch.empty((B, 4 * D), device=DEV)
    L.check(lib().comic_lstm_gates_bwd(ga.data_ptr(), P(c), outs['c_new'].data_ptr(), P(dy),
                                       P(mask), 0.65, P(lens), t, d_dc.data_ptr(),
                                       d_dh.data_ptr(), dg.data_ptr(), B, D, stream()))
    assert_close(dg.cpu().numpy(), dg_ref, 1e-5, 'dg')
    assert_close(d_dc.cpu().numpy(), dc * (1 - live) + dcp_ref, 1e-5, 'dc')
    assert_close(d_dh.cpu().numpy(), dh * (1 - live), 1e-6, 'dh')


ATTN_CASES = [
    # B, M, D, H, Cv, method, prob, tied
    (5, 25, 512, 8, 512, 'add_LN', 'softmax', True),
    (3, 64, 512, 8, 512, 'add_LN', 'softmax', False),
    (3, 196, 512, 8, 512, 'add_LN', 'sigmoid', True),
    (4, 25, 512, 1, 2048, 'add_LN', 'softmax', False),
    (4, 9, 128, 4, 128, 'dot', 'softmax', True),
    (2, 70, 64, 2, 192, 'dot', 'sigmoid', False),
    (3, 25, 1024, 16, 1024, 'add_LN', 'softmax', True)]


@pytest.mark.parametrize('case', ATTN_CASES)
@pytest.mark.parametrize('use_mask', [False, True])
def test_attn_step_fwd_bwd(case, use_mask):
    _attn_step_fwd_bwd(case, use_mask)


@pytest.mark.parametrize('regime', [('offset', 4), ('offset', 32), 'saturated'], ids=str)
def test_attn_step_fwd_bwd_off_unit_scale(regime):
    """The first add_LN case on operands off zero mean and unit scale (tests/regimes.py), against the oracle in float64:
    LayerNorm rows keys + q with a mean of 4 and 32 standard deviations, and gains x 40 (tanh arguments to +-180).
    tests/test_regimes_cpu.py holds the float32 oracle below a quarter of these bars on the same operands."""
    _attn_step_fwd_bwd(ATTN_CASES[0], True, regime)


def _attn_step_fwd_bwd(case, use_mask, regime=None):
    B, M, D, H, Cv, method, prob, tied = case
    rng = np.random.default_rng(B * M + D)
    cfg = dr.DecoderConfig(rnn_size=D, attn_num_heads=H, attn_alignment_method=method, attn_probability_fn=prob,
                           cnn_fm_projection='tied' if tied else 'independent')
    keys = rng.standard_normal((B, M, D)).astype(np.float32)
    values = keys if tied else rng.standard_normal((B, M, Cv)).astype(np.float32)
    q = rng.standard_normal((B, D)).astype(np.float32)
    p = dict(ln_g=(1 + 0.1 * rng.standard_normal(D)).astype(np.float32),
             ln_b=(0.1 * rng.standard_normal(D)).astype(np.float32),
             v=(rng.standard_normal(D) / math.sqrt(D / H) * 3).astype(np.float32), tau=np.array(2.5, np.float32))
    keep = 0.9
    mask = (rng.random((B, H, M)) < keep).astype(np.float32) if use_mask else None
    if regime == 'saturated':
        p['ln_g'] = p['ln_g'] * np.float32(regimes.LN_GAIN_SCALE)
    elif regime is not None:
        keys = regimes.offset(keys, regime[1] * math.sqrt(2.0))     # keys + q has standard deviation sqrt(2)
        values = keys if tied else values
    dev_ops = keys, values, q, p, mask                              # what the device gets: float32
    if regime is not None:                                          # the reference in float64 on the same operands
        keys, values, q, mask = (None if x is None else x.astype(np.float64) for x in (keys, values, q, mask))
        p = {k: v.astype(np.float64) for k, v in p.items()}
    alpha_ref, ac = dr.attention_scores(p, cfg, keys, q)
    alpha_d_ref = dr.dropout(alpha_ref, mask, keep)
    ctx_ref = dr.context(cfg, alpha_d_ref, values)
    ref_ops = keys, values, q, p, mask
    keys, values, q, p, mask = dev_ops
    d = L.AttnDesc(B=B, M=M, D=D, H=H, Cv=Cv, method=0 if method == 'add_LN' else 1,
                   prob=0 if prob == 'softmax' else 1, tied=int(tied))
    dk = dev(keys)
    dvv = dk if tied else dev(values)
    dq_in = dev(q)
    dp = {k: dev(v.reshape(-1)) for k, v in p.items()}
    alpha = torch.empty((B, H, M), device=DEV); alpha_d = torch.empty((B, H, M), device=DEV)
    ctx = torch.empty((B, Cv), device=DEV)
    dmask = dev(mask) if use_mask else None
    L.check(lib().comic_attn_step_fwd(C.byref(d), dk.data_ptr(), dvv.data_ptr(), dq_in.data_ptr(),
                                      dp['ln_g'].data_ptr(), dp['ln_b'].data_ptr(), dp['v'].data_ptr(),
                                      dp['tau'].data_ptr(), L.ptr(dmask), keep, alpha.data_ptr(), alpha_d.data_ptr(),
                                      ctx.data_ptr(), stream()), 'attn_fwd')
    sync()
    ew = True if regime == 'saturated' else None                     # element-wise as well where tanh saturates
    for name, got, ref in (('alpha', alpha, alpha_ref), ('alpha_d', alpha_d, alpha_d_ref), ('ctx', ctx, ctx_ref)):
        if regime is not None:
            print('  %s %-8s err %.3e  bar 1.0e-04' % (regime, name, rel_err(got.cpu().numpy(), ref)))
        assert_close(got.cpu().numpy(), ref, 1e-4, name, elementwise=ew)
    # ---- backward vs the oracle's analytic backward ----
    dctx = rng.standard_normal((B, Cv)).astype(np.float32)
    dmap = (0.01 * rng.standard_normal((B, M))).astype(np.float32)
    dctx_dev, dmap_dev = dctx, dmap
    keys, values, q, p, mask = ref_ops
    if regime is not None:
        dctx, dmap = dctx.astype(np.float64), dmap.astype(np.float64)
    vs = values.reshape(B, M, H, Cv // H)
    dalpha_d = np.einsum('bhd,bmhd->bhm', dctx.reshape(B, H, Cv // H), vs) + dmap[:, None, :]
    dvalues_ref = np.einsum('bhm,bhd->bmhd', alpha_d_ref, dctx.reshape(B, H, Cv // H)).reshape(B, M, Cv)
    dalpha = dalpha_d / alpha_ref.dtype.type(keep) * mask if use_mask else dalpha_d
    grads = {k: np.zeros_like(v) for k, v in p.items()}
    dk_ref, dq_ref = dr._attention_backward(p, cfg, keys, q, ac, alpha_ref, dalpha, grads)
    dq = torch.empty((B, D), device=DEV)
    dkeys = torch.zeros((B, M, D), device=DEV)
    dvalues = dkeys if tied else torch.zeros((B, M, Cv), device=DEV)
    pgrad = torch.zeros((B, 3 * D + 1), device=DEV)
    L.check(lib().comic_attn_step_bwd(C.byref(d), dk.data_ptr(), dvv.data_ptr(), dq_in.data_ptr(),
                                      dp['ln_g'].data_ptr(), dp['ln_b'].data_ptr(), dp['v'].data_ptr(),
                                      dp['tau'].data_ptr(), alpha.data_ptr(), L.ptr(dmask), keep,
                                      P(dctx_dev), P(dmap_dev), dq.data_ptr(), dkeys.data_ptr(),
                                      dvalues.data_ptr(), pgrad.data_ptr(), stream()), 'attn_bwd')
    sync()
    assert_close(dq.cpu().numpy(), dq_ref, F32_RTOL, 'dq')
    if tied:
        assert_close(dkeys.cpu().numpy(), dk_ref + dvalues_ref, F32_RTOL, 'dkeys(tied)')
    else:
        assert_close(dkeys.cpu().numpy(), dk_ref, F32_RTOL, 'dkeys')
        assert_close(dvalues.cpu().numpy(), dvalues_ref, F32_RTOL, 'dvalues')
    if method == 'add_LN':
        pg = pgrad.cpu().numpy().sum(0)
        assert_close(pg[:D], grads['v'], F32_RTOL, 'dv')
        assert_close(pg[D:2 * D], grads['ln_g'], F32_RTOL, 'dln_g')
        assert_close(pg[2 * D:3 * D], grads['ln_b'], F32_RTOL, 'dln_b')
        assert abs(pg[3 * D] - grads['tau']) <= F32_RTOL * max(1e-3, abs(float(grads['tau']))) + 1e-6, 'dtau'


@pytest.mark.parametrize('V', [258, 25599])
def test_xent_fwd_bwd(V):
    _xent_fwd_bwd(V)


@pytest.mark.parametrize('V', [258, 25599])
def test_xent_fwd_bwd_peaked_logits(V):
    """Logit rows 30 N(0,1) + 200 / - 200 with one dominant entry (tests/regimes.py): expf overflows without the max
    subtraction; an all-equal row (uniform softmax, arg-max 0), a row whose target is its arg-max (loss below float32
    epsilon) and a row whose target lies 150 below the maximum (its probability underflows; the loss is 150)."""
    _xent_fwd_bwd(V, 'peaked')


def _xent_fwd_bwd(V, regime=None):
    rng = np.random.default_rng(V)
    T, B = 7, 5
    logits = (3 * rng.standard_normal((T, B, V))).astype(np.float32)
    lens = np.array([7, 3, 5, 1, 6], np.int32)
    targets = rng.integers(0, V, (B, T)).astype(np.int32)
    wmask = (np.arange(T)[None, :] < lens[:, None]).astype(np.float32)
    coef = (wmask / wmask.sum()).astype(np.float32)
    if regime is not None:
        logits, lens, targets, wmask, coef = exec_ops_ref.xent_operands_peaked(V, T, T, B, np.random.default_rng(V), lens=lens)
    dl = dev(logits)
    loss_rows = torch.empty(T * B, device=DEV); dlog = torch.empty((T, B, V), device=DEV)
    ids = torch.empty((T, B), dtype=torch.int32, device=DEV)
    L.check(lib().comic_xent_fwd_bwd(dl.data_ptr(), P(targets), P(coef),
                                     P(wmask), P(lens), loss_rows.data_ptr(),
                                     dlog.data_ptr(), ids.data_ptr(), T, B, V, stream()))
    live = (np.arange(T)[:, None] < lens[None, :])
    lg = logits * live[..., None]
    lsm = dr.log_softmax(lg.astype(np.float64), -1)
    xent = -np.take_along_axis(lsm, targets.T[..., None], 2)[..., 0] * wmask.T
    np.testing.assert_array_equal(dl.cpu().numpy(), lg)                      # finished rows zeroed
    got = loss_rows.cpu().numpy().reshape(T, B)
    print('  xent rows V=%d %s: err %.3e  element-wise %.3e  bar 1.0e-05, rows %.3g ... %.3g' % (
        V, regime, rel_err(got, xent), elementwise_excess(got, xent, 1.0), xent.min(), xent.max()))
    # element-wise too: the max-norm is relative to the largest row (230 with peaked logits), which hides the small ones
    assert_close(got, xent, 1e-5, 'xent rows', elementwise=True)
    if regime is not None:
        assert got[2, 0] == pytest.approx(150.0, rel=1e-5) and 0 <= got[1, 0] < np.finfo(np.float32).eps
    oh = np.zeros_like(lsm); np.put_along_axis(oh, targets.T[..., None], 1.0, 2)
    assert_close(dlog.cpu().numpy(), (np.exp(lsm) - oh) * coef.T[..., None], 1e-5, 'dlogits', elementwise=regime is not None)
    np.testing.assert_array_equal(ids.cpu().numpy(), lg.argmax(-1))


def test_argmax_ties_lowest_index():
    x = np.zeros((3, 300), np.float32)
    x[0, [7, 100, 299]] = 5; x[1, :] = -1; x[2, 299] = 1
    idx = torch.empty(3, dtype=torch.int32, device=DEV)
    L.check(lib().comic_argmax_rows(P(x), idx.data_ptr(), 3, 300, stream()))
    assert idx.cpu().tolist() == [7, 0, 299]


def test_beam_step_vs_oracle_step():
    _beam_step_vs_oracle_step()


def test_beam_step_peaked_logits():
    """logit rows 30 N(0,1) + 200 / - 200 with a dominant entry (tests/regimes.py), the step restated in float64"""
    _beam_step_vs_oracle_step('peaked')


def _beam_step_vs_oracle_step(regime=None):
    rng = np.random.default_rng(5)
    B, W, V, end = 4, 3, 258, 257
    logits = (2 * rng.standard_normal((B, W, V))).astype(np.float32)
    logits[0, 0, 5] = logits[0, 0, 9] = 40.0            # exact tie -> lower flat index first
    if regime is not None:
        logits = regimes.peaked_logits(np.random.default_rng(5), B * W, V)[0].reshape(B, W, V)
        logits[0, 0, 5] = logits[0, 0, 9] = logits[0, 0].max() + 10
    lp = np.array([[0, -1.5, -2.0]] * B, np.float32); lp[1] = [0, -np.inf, -np.inf]
    fin = np.zeros((B, W), np.int32); fin[2, 1] = 1; fin[3] = 1
    lens = rng.integers(0, 5, (B, W)).astype(np.int64)
    step = dr.log_softmax(logits if regime is None else logits.astype(np.float64), -1)
    row = np.full(V, np.finfo(np.float32).min, np.float32); row[end] = 0
    step = np.where(fin[:, :, None].astype(bool), row[None, None, :], step)
    total = (lp[:, :, None] + step).reshape(B, W * V)
    order = np.argsort(-total, axis=1, kind='stable')[:, :W]
    d_lp, d_fin, d_len = dev(lp), dev(fin), dev(lens)
    word = torch.empty((B, W), dtype=torch.int32, device=DEV); par = torch.empty_like(word)
    sc = torch.empty((B, W), device=DEV)
    L.check(lib().comic_beam_step(P(logits), d_lp.data_ptr(), d_fin.data_ptr(), d_len.data_ptr(),
                                  word.data_ptr(), par.data_ptr(), sc.data_ptr(), B, W, V, end, stream()))
    np.testing.assert_array_equal(word.cpu().numpy(), order % V)
    np.testing.assert_array_equal(par.cpu().numpy(), order // V)
    ref_sc = np.take_along_axis(total, order, 1)
    if regime is not None:
        print('  beam scores %s: err %.3e  element-wise %.3e  bar 1.0e-06' % (
            regime, rel_err(sc.cpu().numpy(), ref_sc), elementwise_excess(sc.cpu().numpy(), ref_sc, 1.0)))
    assert_close(sc.cpu().numpy(), ref_sc, 1e-6, 'beam scores', elementwise=regime is not None)
    bidx = np.arange(B)[:, None]
    pf = fin[bidx, order // V].astype(bool)
    np.testing.assert_array_equal(d_fin.cpu().numpy().astype(bool), pf | (order % V == end))
    np.testing.assert_array_equal(d_len.cpu().numpy(), lens[bidx, order // V] + (~pf))
    assert word.cpu().numpy()[0, 0] == 5 and word.cpu().numpy()[0, 1] == 9


# the last three: GEMM + the single-member split step (D = 96, 1024 < V < 4096, W * V >= 8192), one case per form of its chunk
# top-W: 3 chunks of 1034 columns, 5 per thread x 3 beams = 15 register slots (capacity 16); 2 chunks of 1250, 5 x 5 = 25
# (capacity 40); 5 x 9 = 45 (the rescanning form)
@pytest.mark.parametrize('B,W,V,D', [(4, 3, 258, 128), (5, 8, 9000, 128), (6, 3, 8962, 256), (3, 5, 1000, 64), (4, 3, 2500, 96),
                                     (4, 3, 3100, 96), (4, 5, 2500, 96), (4, 9, 2500, 96)])
def test_beam_step_dense_vs_oracle_step(B, W, V, D):
    _beam_step_dense_vs_oracle_step(B, W, V, D)


@pytest.mark.parametrize('B,W,V,D', [(4, 3, 258, 128), (4, 3, 2500, 96), (5, 8, 9000, 128)])
def test_beam_step_dense_peaked_logits(B, W, V, D):
    """The register-resident form, the single-member split form and the streaming-projection form with W_o scaled so that
    the logits spread like 30 N(0,1) and b_o + 200 (tests/regimes.py): the chunk partials' exp(pmax - mx) underflow for
    most chunks, expf overflows without the max subtraction; a finished beam, an entry whose other beams are at -inf and
    an entry with every beam finished as in the sibling.  The step is restated in float64."""
    _beam_step_dense_vs_oracle_step(B, W, V, D, 'peaked')


def _beam_step_dense_vs_oracle_step(B, W, V, D, regime=None):
    """One beam step from the decoder outputs through the kernels the decode loop uses for the shape (streaming projection
    + chunk top-k + merge; register-resident small step; GEMM + comic_beam_step) against the [TF-1.9] step restated in
    numpy: exact ties between duplicate vocabulary columns (lower flat index first, also across chunks and beams), a
    finished beam, an entry whose other beams are at -inf, an entry with every beam finished."""
    o = exec_ops_ref.dense_beam_operands(B, W, V, D, regime)
    end, y, Wo, bo, lp, fin, lens, logits = (o[k] for k in ('end', 'y', 'Wo', 'bo', 'lp', 'fin', 'lens', 'logits'))
    step = dr.log_softmax(logits, -1)
    row = np.full(V, np.finfo(np.float32).min, np.float32); row[end] = 0
    step = np.where(fin[:, :, None].astype(bool), row[None, None, :], step)
    total = (lp[:, :, None] + step).reshape(B, W * V)
    order = np.argsort(-total, axis=1, kind='stable')[:, :W]
    d_lp, d_fin, d_len = dev(lp), dev(fin), dev(lens)
    word = torch.empty((B, W), dtype=torch.int32, device=DEV); par = torch.empty_like(word)
    sc = torch.empty((B, W), device=DEV)
    nb = int(lib().comic_beam_step_dense_workspace(B, W, D, V))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    L.check(lib().comic_beam_step_dense(P(y), P(Wo), P(bo), d_lp.data_ptr(), d_fin.data_ptr(), d_len.data_ptr(),
                                        word.data_ptr(), par.data_ptr(), sc.data_ptr(), B, W, D, V, end, ws.data_ptr(), nb,
                                        stream()))
    sync()
    ref_sc = np.take_along_axis(total, order, 1)
    got_w, got_p, got_sc = word.cpu().numpy(), par.cpu().numpy(), sc.cpu().numpy()
    # device logits carry ~1e-5 of split-product error: where the oracle's neighbours are closer than that the order may
    # legitimately differ; everything else must agree exactly, and exact ties (duplicate columns, equal beams) must
    # resolve to the lower flat index
    fl = got_p.astype(np.int64) * V + got_w
    for b in range(B):
        for k in range(W):
            if fl[b, k] != order[b, k]:
                assert abs(total[b, fl[b, k]] - ref_sc[b, k]) <= 2e-4 * max(1.0, abs(ref_sc[b, k])), (b, k, fl[b, k], order[b, k])
        assert len(set(fl[b].tolist())) == W
    fin_sc = np.isfinite(ref_sc) & (np.abs(ref_sc) < 1e30)
    if regime is not None:
        print('  dense beam scores %s (%d,%d,%d,%d): |logits| to %.0f, err %.3e  element-wise %.3e  bar 2.0e-04' % (
            regime, B, W, V, D, np.abs(logits).max(), rel_err(np.where(fin_sc, got_sc, 0), np.where(fin_sc, ref_sc, 0)),
            elementwise_excess(np.where(fin_sc, got_sc, 0), np.where(fin_sc, ref_sc, 0), 1.0)))
    # peaked: max|ref| is 17 ... 34 where the sibling's is about 2 and most kept scores lie in 0 ... -2, so element-wise too
    assert_close(np.where(fin_sc, got_sc, 0), np.where(fin_sc, ref_sc, 0), 2e-4, 'beam scores', elementwise=regime is not None)
    dup = {3, 7, V - 5}
    for b in range(B):
        ws_b = [int(x) for x in got_w[b]]
        for k in range(W - 1):
            if ws_b[k] in dup and ws_b[k + 1] in dup and got_p[b, k] == got_p[b, k + 1] and got_sc[b, k] == got_sc[b, k + 1]:
                assert ws_b[k] < ws_b[k + 1], 'tie between duplicate columns must keep the lower index first'
    bidx = np.arange(B)[:, None]
    pf = fin[bidx, got_p].astype(bool)
    np.testing.assert_array_equal(d_fin.cpu().numpy().astype(bool), pf | (got_w == end))
    np.testing.assert_array_equal(d_len.cpu().numpy(), lens[bidx, got_p] + (~pf))
    # an entry with every beam finished keeps its beams (EOS at score + 0), in beam order
    np.testing.assert_array_equal(got_w[B - 1], np.full(W, end))
    np.testing.assert_array_equal(got_p[B - 1], np.argsort(-lp[B - 1], kind='stable'))


def test_gather_tree_matches_oracle():
    rng = np.random.default_rng(6)
    T, B, W, end = 9, 5, 4, 17
    step = rng.integers(0, 18, (T, B, W)).astype(np.int32)
    par = rng.integers(0, W, (T, B, W)).astype(np.int32)
    ml = np.array([9, 4, 0, 12, 1], np.int32)
    out = torch.empty((T, B, W), dtype=torch.int32, device=DEV)
    L.check(lib().comic_gather_tree(P(step), P(par), P(ml), out.data_ptr(),
                                    T, B, W, end, stream()))
    np.testing.assert_array_equal(out.cpu().numpy(), beam_ref.gather_tree(step, par, ml, end))


def test_adam_tf_matches_oracle():
    rng = np.random.default_rng(7)
    n = 100003
    w = rng.standard_normal(n).astype(np.float32); g = rng.standard_normal(n).astype(np.float32)
    m = (0.1 * rng.standard_normal(n)).astype(np.float32); v = (0.1 * rng.random(n)).astype(np.float32)
    dw, dg, dm, dv = dev(w), dev(g), dev(m), dev(v)
    t, lr, l2 = 3, 1e-2, 1e-5
    lr_t = lr * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
    L.check(lib().comic_adam_tf(dw.data_ptr(), dg.data_ptr(), dm.data_ptr(), dv.data_ptr(), n, lr_t, 0.9, 0.999,
                                1e-2, l2, 1.0, stream()))
    g_eff = g + np.float32(l2) * w
    dr.adam_tf_update(w, g_eff, m, v, t, lr, eps=1e-2)
    assert_close(dw.cpu().numpy(), w, 1e-5, 'adam w')
    assert_close(dm.cpu().numpy(), m, 1e-5, 'adam m')
    assert_close(dv.cpu().numpy(), v, 1e-5, 'adam v')


@pytest.mark.parametrize('opt_name', ['adam', 'sgd'])
def test_optimiser_update_by_ranges_equals_one_launch(opt_name):
    """The chunked gradient exchange (trainer.DataParallel.exchange_and_step) updates the flat buffer range by range, each
    range behind its own all-reduce, the status word's range first: the same bits as the one-launch update, `before_range`
    called once per range in order, and a voided step (status word set) skips every range."""
    from comic_amd import decoder as cdec, optim
    from comic_amd.trainer import DataParallel
    spec = cdec.DecoderSpec(M=25, C=2048, Cg=2048)
    outs = []
    for mode in ('flat', 'ranges', 'ranges_void'):
        g = torch.Generator(device='cpu').manual_seed(3)
        PP = cdec.FlatParams(spec.param_shapes(), DEV, status_tail=True)
        GG = cdec.FlatParams(spec.param_shapes(), DEV, status_tail=True)
        PP.data[:PP.numel].copy_(torch.randn(PP.numel, generator=g))
        GG.data[:GG.numel].copy_(torch.randn(GG.numel, generator=g))
        opt = optim.make_optimiser(opt_name, PP)
        seen = []
        for step in range(2):
            if mode == 'flat':
                opt.step(GG, 1e-2, grad_scale=0.5)
            else:
                if mode == 'ranges_void' and step == 1:
                    GG.data[GG.numel] = 1.0
                rng_ = DataParallel.chunk_bounds(GG, 4)[::-1]
                opt.step(GG, 1e-2, grad_scale=0.5, ranges=rng_, before_range=seen.append)
        sync()
        assert mode == 'flat' or seen == [0, 1, 2, 3] * 2
        outs.append((PP.data.clone(), opt.m.data.clone(), opt.v.data.clone(), opt.t))
    assert all(torch.equal(a, b) for a, b in zip(outs[0][:3], outs[1][:3])) and outs[0][3] == outs[1][3] == 2
    opt1 = outs[2]
    assert not torch.equal(opt1[0], outs[0][0])        # the voided second step left the parameters of step 1 ...
    PP = cdec.FlatParams(spec.param_shapes(), DEV, status_tail=True)
    GG = cdec.FlatParams(spec.param_shapes(), DEV, status_tail=True)
    g = torch.Generator(device='cpu').manual_seed(3)
    PP.data[:PP.numel].copy_(torch.randn(PP.numel, generator=g))
    GG.data[:GG.numel].copy_(torch.randn(GG.numel, generator=g))
    o1 = optim.make_optimiser(opt_name, PP)
    o1.step(GG, 1e-2, grad_scale=0.5)
    sync()
    assert torch.equal(opt1[0][:PP.numel], PP.data[:PP.numel])      # ... in every range


def test_gradient_clipping_matches_oracle():
    """clip_gradient_norm (model_base.py:394-401): tf.clip_by_norm per variable on g*gscale + l2*w, then the TF-Adam update;
    variables of one element, of less than a chunk and of several chunks, norms above and below the threshold, and the
    voided-step flag."""
    from comic_amd import decoder as cdec, optim
    rng = np.random.default_rng(11)
    shapes = {'a': (3, 5000), 'b': (700,), 'c': (), 'd': (40000,), 'e': (128, 64)}
    scale_of = {'a': 1.0, 'b': 1e-3, 'c': 50.0, 'd': 0.2, 'e': 1e-2}
    PP = cdec.FlatParams(shapes, DEV, status_tail=True)
    G = PP.like()
    w = {k: rng.standard_normal(shapes[k]).astype(np.float32) for k in shapes}
    g = {k: (scale_of[k] * rng.standard_normal(shapes[k])).astype(np.float32) for k in shapes}
    PP.load(w); G.load(g)
    clip, l2, gs, lr = 2.5, 1e-3, 0.5, 1e-2
    opt = optim.AdamTF(PP, l2_decay=l2, clip_norm=clip)
    opt.step(G, lr, grad_scale=gs)
    got = PP.to_numpy()
    n_clipped = 0
    for k in shapes:
        ge = np.float32(gs) * g[k] + np.float32(l2) * w[k]
        n_clipped += float(np.sqrt((ge.astype(np.float64) ** 2).sum())) > clip
        ge = dr.clip_by_norm(ge, clip)
        wk, m, v = w[k].copy(), np.zeros_like(w[k]), np.zeros_like(w[k])
        dr.adam_tf_update(wk, ge, m, v, 1, lr, eps=1e-2)
        assert_close(got[k], wk, 1e-5, 'clipped adam ' + k)
    assert 2 <= n_clipped < len(shapes)                      # both sides of the threshold are exercised
    # a voided step: neither the clip nor the update touches anything
    G.status.fill_(1.0)
    before, gbefore = PP.data.clone(), G.data.clone()
    opt.step(G, lr, grad_scale=gs)
    assert torch.equal(PP.data, before) and torch.equal(G.data, gbefore)


def test_momentum_tf_matches_oracle():
    """--optimiser sgd: tf.train.MomentumOptimizer(0.9, use_nesterov=False) (model_base.py:867-880), two updates."""
    rng = np.random.default_rng(8)
    n = 70001
    w = rng.standard_normal(n).astype(np.float32)
    acc = np.zeros(n, np.float32)
    dw, dacc = dev(w), dev(acc)
    lr, l2 = 1e-2, 1e-5
    for it in range(2):
        g = rng.standard_normal(n).astype(np.float32)
        L.check(lib().comic_momentum_tf(dw.data_ptr(), dev(g).data_ptr(), dacc.data_ptr(), n, lr, 0.9, l2, 0.5, stream()))
        dr.momentum_tf_update(w, np.float32(0.5) * g + np.float32(l2) * w, acc, lr)
    assert_close(dw.cpu().numpy(), w, 1e-6, 'momentum w')
    assert_close(dacc.cpu().numpy(), acc, 1e-6, 'momentum accum')


def test_legacy_encoder_head_matches_oracle():
    """--legacy image embedding (model_base.py:80-91): LN_tanh + linear(1024) forward and parameter gradients."""
    from comic_amd import encoder_head
    rng = np.random.default_rng(9)
    B, C_ = 6, 1024
    net = (rng.standard_normal((B, C_)) * 1.5 + 0.2).astype(np.float32)
    p = encoder_head.init_params(C_, seed=1)
    p['ln_gamma'] = rng.uniform(0.5, 1.5, C_).astype(np.float32)
    p['ln_beta'] = (0.1 * rng.standard_normal(C_)).astype(np.float32)
    head = encoder_head.LegacyEncoderHead(C_, p, DEV)
    out = head.forward(dev(net))
    ref, cache = dr.legacy_head_forward(p, net)
    assert_close(out.cpu().numpy(), ref, 1e-3, 'legacy im_embed')
    d = rng.standard_normal(ref.shape).astype(np.float32)
    g = head.backward(dev(d)).to_numpy()
    gref = dr.legacy_head_backward(p, cache, d)
    for k in gref:
        assert_close(g[k], gref[k], 1e-3, 'legacy d ' + k)
    assert set(head.export_params()) == {'Model/encoder/LN_tanh/beta', 'Model/encoder/LN_tanh/gamma',
                                         'Model/encoder/im_embed/weight'}


@pytest.mark.parametrize('r', regimes.OFFSETS)
@pytest.mark.parametrize('C_', [192, 2048])
def test_ln_tanh_kernels_on_non_negative_rows(C_, r):
    """comic_ln_tanh_fwd / comic_ln_tanh_bwd_rows on their own operands: pooled post-ReLU features are non-negative, so
    the head's LayerNorm rows have a mean of several standard deviations (here 4 and 32).  y and xhat at the bar of the
    same formula in the attention step (1e-4), the per-row gradient terms at 1e-3 on the float32 roundings of the
    reference's saved tensors; outputs NaN before the launch."""
    B = 5
    rng = np.random.default_rng(C_ + r)
    x = regimes.nonneg_offset(rng, (B, C_), r)
    gamma = rng.uniform(0.5, 1.5, C_).astype(np.float32)
    beta = (0.1 * rng.standard_normal(C_)).astype(np.float32)
    dy = rng.standard_normal((B, C_)).astype(np.float32)
    x64 = x.astype(np.float64)
    mean = x64.mean(1, keepdims=True)
    xhat_ref = (x64 - mean) / np.sqrt(((x64 - mean) ** 2).mean(1, keepdims=True) + 1e-12)
    y_ref = np.tanh(xhat_ref * gamma + beta)
    y, xhat, pg, pb = (torch.full((B, C_), float('nan'), device=DEV) for _ in range(4))
    L.check(lib().comic_ln_tanh_fwd(P(x), P(gamma), P(beta), y.data_ptr(), xhat.data_ptr(), B, C_, 1e-12, stream()), 'ln_tanh_fwd')
    sync()
    for name, got, ref in (('y', y, y_ref), ('xhat', xhat, xhat_ref)):
        print('  LN_tanh C=%d offset(%d) %-5s err %.3e  bar 1.0e-04' % (C_, r, name, rel_err(got.cpu().numpy(), ref)))
        assert_close(got.cpu().numpy(), ref, 1e-4, name, elementwise=True)
    y32, xh32 = y_ref.astype(np.float32), xhat_ref.astype(np.float32)
    L.check(lib().comic_ln_tanh_bwd_rows(P(dy), P(y32), P(xh32), pg.data_ptr(), pb.data_ptr(), B, C_, stream()), 'ln_tanh_bwd_rows')
    sync()
    t = dy.astype(np.float64) * (1.0 - y32.astype(np.float64) ** 2)
    assert_close(pg.cpu().numpy(), t * xh32, F32_RTOL, 'd gamma rows')
    assert_close(pb.cpu().numpy(), t, F32_RTOL, 'd beta rows')


def test_process_decode_pool_equals_thread_decode(tmp_path):
    """inputs.DecodePool (spawned workers decoding JPEGs into shared-memory staging, registered as pinned memory) feeds
    the device preprocessing the same bytes as the in-process PIL decode: identical output tensors, blocks recycled
    over several batches, an image larger than its slot is refused with a clear error."""
    from PIL import Image
    from comic_amd import inputs
    rng = np.random.default_rng(4)
    paths = []
    for i, (h, w) in enumerate([(48, 64), (33, 50), (64, 64), (20, 31), (57, 40)]):
        p = str(tmp_path / ('%d.jpg' % i))
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p, quality=92)
        paths.append(p)
    params = [(bool(i & 1), i, 2 * i) for i in range(len(paths))]
    pre = inputs.DevicePreprocessor(DEV, 224, 224)
    want = pre([inputs.decode_image(p) for p in paths], params).cpu()
    pool = inputs.DecodePool(2, blocks=2, slot_bytes=64 * 64 * 3, max_batch=8)
    try:
        for _ in range(5):                                   # more batches than blocks: they are recycled
            got = pre.finish(pre.pack_paths(pool, paths, params)).cpu()
            assert torch.equal(got, want)
        big = str(tmp_path / 'big.jpg')
        Image.fromarray(rng.integers(0, 256, (80, 80, 3), dtype=np.uint8)).save(big)
        with pytest.raises(ValueError, match='loader slot'):
            pre.finish(pre.pack_paths(pool, [big], [(False, 0, 0)]))
    finally:
        pool.close()
