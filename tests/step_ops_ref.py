"""Float64 references of the fused and streaming LSTM step kernels (tests/test_gpu_step_ops.py), on the float32 operands:
the step and its two backward forms (csrc/decoder_fused.hip), the decode loops' operand gather, the bf16 hi / lo
fragment layout and the split arithmetic of the streaming step (csrc/lstm_stream.hip, csrc/lstm_prep.h).

Every reference takes `mut`, the name of ONE deliberate mistake (MUTANTS_*): tests/test_step_ops_ref_cpu.py holds each
mutant against the true reference under the GPU test's own criterion (`within`) and requires it to fail there, so a
kernel with that mistake cannot pass.  The cell formulas are held to the oracle's lstm_cell / _lstm_backward."""
import numpy as np

from oracle import decoder_ref as dr
from oracle.cnn_ref import bf16_round
from tests import regimes
from tests.exec_ops_ref import GATES_TOL, f64
from tests.gpu_util import elementwise_excess, rel_err

KEEP = 0.9
T_STEP = 2                  # the step's t; lens mixes finished (lens <= t) and live rows
# The streaming step multiplies bf16 hi / lo halves (hi*hi + hi*lo + lo*hi, fp32 accumulation, K-slices added in slice
# order): its bar is 4 x the largest error of a float32 numpy emulation of exactly that arithmetic against float64, the
# quarter rule of exec_ops_ref.py sized from the reference side.  Measured by test_stream_bar_is_four_times_the_emulation
# as max|a - b| / max|b| (the measure of exec_ops_ref's quarter rule), c2 / h2 (= y) per STREAM_SHAPES row; in brackets
# the element-wise measure max |a - b| / (|b| + rms(b)) of the same emulation:
#   (33,3,16,8,8)         2.29e-6 / 3.53e-6   [5.73e-6 / 9.56e-6]
#   (48,3,48,24,24)       2.30e-6 / 5.97e-6   [6.83e-6 / 1.33e-5]
#   (129,3,48,56,56)      2.84e-6 / 8.15e-6   [9.23e-6 / 2.17e-5]
#   (150,3,48,184,184)    2.90e-6 / 1.04e-5   [1.29e-5 / 2.66e-5]
#   (256,8,512,256,2048)  3.47e-6 / 9.01e-6   [1.14e-5 / 2.23e-5]
# largest 1.04e-5 -> 4 x = 4.2e-5, below the 5e-5 that test_gemm_f32_stream allows the same product.  The GPU test
# applies the bar to both measures; of the element-wise one the emulation alone uses 2.66e-5 / 4.2e-5 = 63 % (four times
# that figure would pass the 5e-5 cap, so the bar stays at the max-norm figure and the kernel gets the remaining 37 %).
STREAM_TOL = 4.2e-5
STREAM_TOL_CAP = 5e-5

# B, D, E + A of the fused step; the same geometries as (B, E, A, D) of the input gradient, E | A inside a 16-feature
# tile everywhere and, in the second row of each pair, A | D too (E + A is a multiple of 16 in the first)
FUSED_SHAPES = [(1, 4, 4), (17, 36, 32), (16, 128, 320), (67, 512, 2304)]
GRAD_SHAPES = [(1, 1, 3, 4), (17, 10, 22, 36), (17, 10, 18, 36), (16, 70, 250, 128), (16, 70, 254, 128),
               (67, 250, 2054, 512), (67, 250, 2058, 512)]
QGRAD_SHAPES = [(1, 16), (17, 48), (67, 512)]
INFER_FUSED_SHAPES = [(R, W, D, E, A) for D, E, A in ((36, 20, 12), (128, 64, 128)) for R, W in ((5, 1), (12, 3), (32, 8))]
# R, W, D, E, A -> K-slices of the streamed product
STREAM_SHAPES = [((33, 3, 16, 8, 8), 1), ((48, 3, 48, 24, 24), 3), ((129, 3, 48, 56, 56), 5), ((150, 3, 48, 184, 184), 7),
                 ((256, 8, 512, 256, 2048), 8)]
BOTH_SHAPE = (48, 3, 48, 24, 24)            # served by the streaming and (forced) by the fused step
# B, W, V, D, E, A of the beam step that prepares the next operand rows: merge kernel; small step (Wd % 32 != 0 in both)
PREP_SHAPES = [(11, 3, 4300, 128, 8, 8), (5, 8, 258, 64, 8, 16)]

GATE_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
MUTANTS_STEP = ['swap%d%d' % p for p in GATE_PAIRS] + ['no_forget_bias', 'keep', 'fin', 'k_tail']
MUTANTS_STREAM = ['swap%d%d' % p for p in GATE_PAIRS] + ['no_forget_bias', 'k_tail', 'last_slice']
MUTANTS_GATHER = ['clamp_hi', 'clamp_lo', 'src_is_r', 'bad_id']
MUTANTS_INPUT_GRAD = ['keep', 'carry', 'k_tail']
MUTANTS_QGRAD = ['keep', 'fin', 'k_tail']


def figure(got, ref):
    """the smallest tolerance at which `within` holds: max-norm and element-wise measure of gpu_util.assert_close"""
    return max(rel_err(got, ref), elementwise_excess(got, ref, 1.0))


def within(got, ref, tol):
    """the GPU test's criterion: gpu_util.assert_close(got, ref, tol, elementwise=True) as a predicate"""
    got = np.asarray(got, np.float64)
    return bool(np.isfinite(got).all() and rel_err(got, ref) <= tol and elementwise_excess(got, ref, tol) <= 1.0)


def lens_for(B):
    """finished (lens <= T_STEP) and live rows; the LAST row, which lies in the ragged tail tile, is finished"""
    lens = np.array([3, 1, 5, 2, 9, 2, 4] * (B // 7 + 1), np.int32)[:B]
    if B > 1:
        lens[B - 1] = 1
    return lens


# ------------------------------------------------------------------------------------------------- inputs ------------
def gate_bias(rng, D):
    """a different offset per gate block: an i / j / f / o mix-up or a dropped forget bias moves the gates by O(0.1)"""
    return (np.repeat([0.3, -0.5, 0.7, -0.2], D) + 0.1 * rng.standard_normal(4 * D)).astype(np.float32)


def saturate_step(b, c):
    """regime 'saturated' (tests/regimes.py) of one step's operands: the gate biases uniform over +-100 (both ends
    present), so that the pre-activations [x;h] K + b cross every branch of the sigmoid / tanh forms and the expf overflow
    point while the product keeps its normal-regime rounding; the previous cell states scaled to reach +-50"""
    bs = np.random.default_rng(len(b)).uniform(-regimes.PEAK, regimes.PEAK, len(b))
    bs[0], bs[-1] = regimes.PEAK, -regimes.PEAK
    return bs.astype(np.float32), regimes.saturate(c, regimes.CELL_PEAK)


def step_inputs(B, D, EA, seed=None, regime=None):
    """regime: None or 'saturated'; the draws are those of regime None"""
    Wd = EA + D
    rng = np.random.default_rng(1000 * B + D + EA if seed is None else seed)
    inp = _step_draws(rng, B, D, Wd)
    if regime is not None:
        assert regime == 'saturated', regime
        inp['b'], inp['c'] = saturate_step(inp['b'], inp['c'])
    return inp


def _step_draws(rng, B, D, Wd):
    return dict(K=(rng.standard_normal((Wd, 4 * D)) / np.sqrt(Wd)).astype(np.float32), b=gate_bias(rng, D),
                xh=rng.standard_normal((B, Wd)).astype(np.float32),
                c=rng.standard_normal((B, D)).astype(np.float32), h=(0.5 * rng.standard_normal((B, D))).astype(np.float32),
                mask=(rng.random((B, D)) < KEEP).astype(np.float32), lens=lens_for(B))


def grad_inputs(B, E, A, D, regime=None):
    """regime 'saturated': the gate gradients of saturated cells, exact zeros but for one element in eight"""
    Wd = E + A + D
    rng = np.random.default_rng(B + 7 * E + 11 * A + 13 * D)
    inp = _grad_draws(rng, B, E, A, D, Wd)
    if regime is not None:
        assert regime == 'saturated', regime
        inp['dg'] = inp['dg'] * (np.random.default_rng(Wd).random(inp['dg'].shape) < 0.125).astype(np.float32)
    return inp


def _grad_draws(rng, B, E, A, D, Wd):
    return dict(K=(rng.standard_normal((Wd, 4 * D)) / np.sqrt(Wd)).astype(np.float32),
                dg=rng.standard_normal((B, 4 * D)).astype(np.float32),
                mask=(rng.random((B, E + A)) < KEEP).astype(np.float32),
                datt=rng.standard_normal((B, A)).astype(np.float32), dh=(2 + rng.standard_normal((B, D))).astype(np.float32),
                lens=lens_for(B))


def qgrad_inputs(B, D, regime=None):
    rng = np.random.default_rng(3 * B + D)
    st = step_inputs(B, D, 16, seed=B + D, regime=regime)
    fw = lstm_step_ref(st['xh'], st['K'], st['b'], st['c'], None, None, 1.0, None, 0)
    return dict(Wq=(rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32),
                dq=rng.standard_normal((B, D)).astype(np.float32), dy=rng.standard_normal((B, D)).astype(np.float32),
                gates_act=fw['gates_act'].astype(np.float32), c_new=fw['c_new'].astype(np.float32), c=st['c'],
                mask=st['mask'], dc=rng.standard_normal((B, D)).astype(np.float32),
                dh=(1 + rng.standard_normal((B, D))).astype(np.float32), lens=st['lens'])


def infer_inputs(R, W, D, E, A, V=37, seed=None, regime=None):
    """one decode step's sources: non-identity parents with -1 and W + 3 (the clamp), the ids -1 and V (zero rows);
    regime 'saturated': b and c as in step_inputs"""
    inp = _infer_draws(R, W, D, E, A, V, seed)
    if regime is not None:
        assert regime == 'saturated', regime
        inp['b'], inp['c'] = saturate_step(inp['b'], inp['c'])
    return inp


def _infer_draws(R, W, D, E, A, V, seed):
    rng = np.random.default_rng(R + 3 * W + 5 * D + E + A if seed is None else seed)
    Wd = E + A + D
    ids = rng.integers(0, V, R).astype(np.int32)
    parent = rng.integers(0, W, R).astype(np.int32)
    parent[0] = -1
    ids[R // 2] = -1
    ids[R - 1] = V
    if W > 1:
        parent[R - 1] = W + 3
        parent[1] = W + 3         # clamps to the entry's last beam; one too far would be the next entry's first row
        parent[W] = 1             # a row of the second entry reads a sibling
    return dict(table=rng.standard_normal((V, E)).astype(np.float32), ids=ids, parent=parent if W > 1 else None,
                att=rng.standard_normal((R, A)).astype(np.float32), h=(0.5 * rng.standard_normal((R, D))).astype(np.float32),
                c=rng.standard_normal((R, D)).astype(np.float32),
                K=(rng.standard_normal((Wd, 4 * D)) / np.sqrt(Wd)).astype(np.float32), b=gate_bias(rng, D), V=V)


# ------------------------------------------------------------------------------------------------- LSTM step ---------
def _tail(n, unit):
    return n % unit or unit


def lstm_step_ref(xh, K, b, c_prev, h_prev, mask, keep, lens, t, dtype=np.float64, mut=None, g=None):
    """g = [x;att;h] K + b (or the given product); BasicLSTMCell with forget bias 1; output dropout; finished rows
    (t >= lens[b]) keep c_prev / h_prev.  -> gates_act [B,4D], c_new, h_new, y, c_state, h_state (= the xh_next columns)"""
    cast = (lambda x: None if x is None else np.asarray(x, dtype))
    xh, K, b, c_prev, h_prev, mask = (cast(x) for x in (xh, K, b, c_prev, h_prev, mask))
    if g is None:
        Wd = xh.shape[1]
        kk = Wd - _tail(Wd, 16) if mut == 'k_tail' else Wd
        g = xh[:, :kk] @ K[:kk]
    g = cast(g) + (0 if b is None else b)
    D = g.shape[1] // 4
    gs = [g[:, k * D:(k + 1) * D] for k in range(4)]
    if mut and mut.startswith('swap'):
        p, q = int(mut[4]), int(mut[5])
        gs[p], gs[q] = gs[q], gs[p]
    c = np.zeros_like(gs[0]) if c_prev is None else c_prev
    h = np.zeros_like(gs[0]) if h_prev is None else h_prev
    one = dtype(0.0 if mut == 'no_forget_bias' else 1.0)
    si, tj, sf, so = dr.sigmoid(gs[0]), np.tanh(gs[1]), dr.sigmoid(gs[2] + one), dr.sigmoid(gs[3])
    c2 = c * sf + si * tj
    h2 = np.tanh(c2) * so
    y = h2 if mask is None else (h2 * mask if mut == 'keep' else dr.dropout(h2, mask, keep))
    fin = np.zeros((g.shape[0], 1), bool) if (lens is None or mut == 'fin') else (t >= np.asarray(lens))[:, None]
    return dict(gates_act=np.concatenate([si, tj, sf, so], 1), c_new=c2, h_new=h2, y=y, c_state=np.where(fin, c, c2),
                h_state=np.where(fin, h, h2))


def lstm_bwd_ref(gates_act, c_prev, c_new, dy_total, mask, keep, lens, t, dc, dh, mut=None, dtype=np.float64):
    """backward of the output dropout and of the cell (dr._lstm_backward) with the finished-row rule of
    lstm_gates_bwd: -> dg [B,4D], dc_state, dh_state"""
    cast = (lambda x: None if x is None else np.asarray(x, dtype))
    ga, c_new, dy_total, dc, dh, mask = (cast(x) for x in (gates_act, c_new, dy_total, dc, dh, mask))
    D = c_new.shape[1]
    c = np.zeros_like(c_new) if c_prev is None else cast(c_prev)
    live = np.ones((len(c_new), 1), dtype) if (lens is None or mut == 'fin') else (t < np.asarray(lens))[:, None].astype(dtype)
    dyv = dy_total if mask is None else (dy_total * mask if mut == 'keep' else dr.dropout(dy_total, mask, keep))
    gates = tuple(ga[:, k * D:(k + 1) * D] for k in range(4)) + (np.tanh(c_new),)
    dg, dcp = dr._lstm_backward(None, gates, c, dc * live, dh * live + dyv, D)
    return dict(dg=dg, dc=dc * (1 - live) + dcp, dh=dh * (1 - live))


def lstm_grad_ref(dq, Wq, gates_act, c_prev, c_new, dy, mask, keep, lens, t, dc, dh, mut=None, dtype=np.float64):
    """dy_total = dy + dq W_q^T, then lstm_bwd_ref"""
    dq, Wq = np.asarray(dq, dtype), np.asarray(Wq, dtype)
    kk = Wq.shape[1] - (16 if mut == 'k_tail' else 0)
    tot = dq[:, :kk] @ Wq[:, :kk].T
    if dy is not None:
        tot = tot + np.asarray(dy, dtype)
    return lstm_bwd_ref(gates_act, c_prev, c_new, tot, mask, keep, lens, t, dc, dh, mut, dtype)


def input_grad_ref(dg, K, mask, keep, datt, dh, lens, t, carry, E, A, dtype=np.float64, mut=None):
    """d [x;att;h] = dg K^T; input-dropout backward on the x and att columns; datt = (carry && !finished ? 0 : old) + v;
    dh accumulated.  -> demb [B,E], datt [B,A], dh [B,D]"""
    cast = (lambda x: None if x is None else np.asarray(x, dtype))
    dg, K, mask, datt, dh = (cast(x) for x in (dg, K, mask, datt, dh))
    kk = dg.shape[1] - (16 if mut == 'k_tail' else 0)
    d = dg[:, :kk] @ K[:, :kk].T
    EA = E + A
    dx = d[:, :EA] if mask is None else (d[:, :EA] * mask if mut == 'keep' else dr.dropout(d[:, :EA], mask, keep))
    fin = np.zeros((len(dg), 1), bool) if lens is None else (t >= np.asarray(lens))[:, None]
    old = datt if (not carry or mut == 'carry') else np.where(fin, datt, 0)
    return dict(demb=dx[:, :E], datt=old + dx[:, E:], dh=dh + d[:, EA:])


# ------------------------------------------------------------------------------------------------- gather ------------
def gather_ref(table, ids, parent, W, att, h, c, V, mut=None):
    """row r reads source row (r / W) W + clamp(parent[r], 0, W - 1) (parent None: r); an id outside [0, V) embeds as
    zeros.  -> x [R, E+A+D], c_in [R, D]; copies, bit for bit"""
    R = len(ids)
    r = np.arange(R)
    if parent is None or mut == 'src_is_r':
        src = r
    else:
        lo, hi = (1 if mut == 'clamp_lo' else 0), (W if mut == 'clamp_hi' else W - 1)
        src = np.minimum((r // W) * W + np.clip(parent, lo, hi), R - 1)
    ok = (ids >= 0) & (ids < V)
    emb = table[np.clip(ids, 0, V - 1)]
    if mut != 'bad_id':
        emb = np.where(ok[:, None], emb, np.float32(0))
    return np.concatenate([emb, att[src], h[src]], 1).astype(np.float32), c[src].astype(np.float32)


# ------------------------------------------------------------------------------------------------- fragments ---------
def split_hi_lo(x):
    """hi = bf16_rne(x), lo = bf16_rne(x - hi), as float32"""
    x = np.ascontiguousarray(x, np.float32)
    hi = bf16_round(x)
    return hi, bf16_round(x - hi)


def _bits(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def frag_shape(R, Kin):
    return ((R + 15) // 16, (Kin + 31) // 32, 2, 64, 8)


def frag_encode(x):
    """x [R, Kin] float32 -> uint16 [16-row tile][k32-step][hi, lo][lane][8]: lane (r % 16) + 16 (seg % 4) holds the 8
    features 32 s + 8 (seg % 4) ... of row r; rows beyond R and features beyond Kin are zeros"""
    R, Kin = x.shape
    T, KS = frag_shape(R, Kin)[:2]
    xp = np.zeros((T * 16, KS * 32), np.float32)
    xp[:R, :Kin] = x
    out = np.empty((T, KS, 2, 64, 8), np.uint16)
    for hl, part in enumerate(split_hi_lo(xp)):
        b = _bits(part).reshape(T, 16, KS, 4, 8)                    # tile, fr, s, fg, j
        out[:, :, hl] = b.transpose(0, 2, 3, 1, 4).reshape(T, KS, 64, 8)
    return out


def frag_rows(frag):
    """the inverse permutation: uint16 [T][KS][2][64][8] -> bf16 bit patterns hi, lo [16 T, 32 KS]"""
    T, KS = frag.shape[:2]
    b = frag.reshape(T, KS, 2, 4, 16, 8).transpose(2, 0, 4, 1, 3, 5)    # hl, tile, fr, s, fg, j
    return b[0].reshape(T * 16, KS * 32), b[1].reshape(T * 16, KS * 32)


def frag_decode(frag, R, Kin):
    """-> hi, lo [R, Kin] as float32"""
    return tuple((p[:R, :Kin].astype(np.uint32) << 16).view(np.float32) for p in frag_rows(np.ascontiguousarray(frag)))


# ------------------------------------------------------------------------------------------------- streaming ---------
def stream_slices(N, Kin):
    """k32-steps per K-slice and the slice count of the streamed product with N columns (lstm_slices)"""
    KS, chunks = (Kin + 31) // 32, N // 64
    s = min(8, max(1, 256 // chunks))
    n = min(16, (KS + s - 1) // s)
    return n, (KS + n - 1) // n


def stream_product(x, K, emulate, mut=None):
    """x K over the K-slices of the streaming kernel.  emulate: float32 hi*hi + hi*lo + lo*hi per slice, the slices
    added in slice order in float32; else float64 on the float32 operands."""
    Wd, N = K.shape
    n, S = stream_slices(N, Wd)
    if mut == 'k_tail':
        Wd -= _tail(Wd, 32)
    if mut == 'last_slice':
        S -= 1
    if not emulate:
        kk = min(Wd, S * n * 32)
        return f64(x)[:, :kk] @ f64(K)[:kk]
    xh, xl = split_hi_lo(x)
    kh, kl = split_hi_lo(K)
    g = np.zeros((x.shape[0], N), np.float32)
    for s in range(S):
        k = slice(s * n * 32, min(Wd, (s + 1) * n * 32))
        g = g + ((xh[:, k] @ kh[k] + xh[:, k] @ kl[k]) + xl[:, k] @ kh[k])
    assert g.dtype == np.float32
    return g


def infer_step_ref(inp, W, emulate=False, mut=None, gather_mut=None):
    """gather + step of one decode call: -> x, c_in (float32 copies) and the float64 (or emulated float32) cell"""
    x, c_in = gather_ref(inp['table'], inp['ids'], inp['parent'], W, inp['att'], inp['h'], inp['c'], inp['V'], gather_mut)
    smut = mut if mut in ('k_tail', 'last_slice') else None
    g = stream_product(x, inp['K'], emulate, smut)
    out = lstm_step_ref(None, None, inp['b'], c_in, None, None, 1.0, None, 0, np.float32 if emulate else np.float64,
                        None if smut else mut, g=g)
    return x, c_in, out
