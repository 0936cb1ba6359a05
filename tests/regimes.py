"""Operand regimes off the zero-mean, unit-scale draws of the normal tests, and the rule that sets their bars.

Every other test input is N(0, 1) or a small multiple of it.  A kernel that restates a softmax, a LayerNorm, a tanh or a
sigmoid with a shortcut can be exact there and wrong on operands a trained model produces.  Each regime exists to break
one such shortcut; run the regime of the formula you touched:

  regime        operands                                            shortcut it breaks                  restatement that must fail
  ------------  --------------------------------------------------  ----------------------------------  --------------------------------
  offset(r)     LayerNorm rows with mean = r * std, r in {4, 32}    one-pass variance E[z^2] - E[z]^2   one_pass_layer_norm
  features      |N(0,1)| maps, W_m + delta * 1 1^T (whole decoder)  the same, through the time loops    (the offset case at oracle level)
  peaked        logit rows 30 N(0,1) +- 200 with a dominant entry   missing max subtraction             softmax_no_max
                ... a target more than 100 below the max            probability underflow in the loss   loss_from_probability
                ... chunks that are -inf throughout                 -inf - -inf in chunk merges         lse_merge(guard=False)
                ... a first token above p, p met at the last token  quantised / rounded top-p mass      top_p_keep(dtype=float32)
  saturated     gate pre-activations to +-100, cells to +-50,       expf overflow in sigmoid / tanh     tanh_exp_ratio
                attention gains x 40

The restatements live in this file (numpy float32) and tests/test_regimes_cpu.py shows that each lands outside the bar in
its regime, so the GPU cases can fail.

Bar rule (bar()): a kernel is held to the bar its op has in the normal regime.  Only where the float32 restatement of the
REFERENCE on the same operands already misses a quarter of that bar is the bar 4 x that restatement's error against
float64: the factor covers another summation order and the <= 2 ulp hardware exp / rcp.  Both figures come from the
reference side, never from the code under test.  test_regimes_cpu.py caps the restatement's error at a quarter of the op
bar (a tenth of the step bar for whole-decoder tests), so with the parameters below the op's own bar holds everywhere."""
import math

import numpy as np

OFFSETS = (4, 32)
PEAK = 100.0                # |pre-activation| of the saturated regime: expf(88.7) is the last finite float32
CELL_PEAK = 50.0            # previous cell states of the saturated regime
LN_GAIN_SCALE = 40.0        # attention ln_g of the saturated regime
LOGIT_SCALE, LOGIT_SHIFT = 30.0, 200.0
HALF_NORMAL_MEAN, HALF_NORMAL_STD = math.sqrt(2 / math.pi), math.sqrt(1 - 2 / math.pi)


def bar(op_bar, fp32_err):
    """the bar of one (op, regime) pair from the op's normal bar and the float32 restatement's error against float64"""
    return op_bar if fp32_err <= op_bar / 4 else 4 * fp32_err


def rel_err(got, ref):
    """max|a - b| / max|b| (the measure of gpu_util.rel_err, restated so that this file needs numpy alone)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))


def row_ratio(z):
    """|mean| / std over the last axis of every row"""
    z = np.asarray(z, np.float64)
    return np.abs(z.mean(-1)) / z.std(-1)


# ------------------------------------------------------------------------------------------------- offset ------------
def offset(x, r):
    """rows of unit standard deviation moved to mean r (float32, as the kernels get them)"""
    return (np.asarray(x, np.float32) + np.float32(r)).astype(np.float32)


def nonneg_offset(rng, shape, r, s=1.5):
    """|N(0,1)| s + c >= 0 with c such that a row's mean is r times its standard deviation: pooled post-ReLU features"""
    c = s * (r * HALF_NORMAL_STD - HALF_NORMAL_MEAN)
    assert c >= 0
    return (np.abs(rng.standard_normal(shape)) * s + c).astype(np.float32)


# ------------------------------------------------------------------------------------------------- features ----------
def features_batch(rng, B, M, C, Cg):
    """post-ReLU statistics of the feature map and the image embedding"""
    return np.abs(rng.standard_normal((B, M, C))).astype(np.float32), np.abs(rng.standard_normal((B, Cg))).astype(np.float32)


def rank_one(W, delta):
    """W + delta 1 1^T: every key row gets the common offset delta * sum_c fm[m, c]"""
    return (np.asarray(W, np.float64) + delta).astype(np.float32)


def solve_delta(ratio_of, r, delta0, rounds=4):
    """delta at which ratio_of(delta), the median |mean| / std of the oracle's own z = keys + q, is r.  The ratio is close
    to linear in delta (q and the spread of z move a little with it): a few proportional steps settle it."""
    delta = delta0
    for _ in range(rounds):
        got = ratio_of(delta)
        if abs(got / r - 1) < 0.02:
            break
        delta *= r / got
    return delta


# ------------------------------------------------------------------------------------------------- peaked ------------
def peaked_logits(rng, rows, V, equal_row=None, argmax_row=None, underflow_row=None, targets=None):
    """-> logits [rows, V] float32, targets [rows] int32.  Rows are 30 N(0,1) + 200 (even rows) or - 200 (odd rows) with one
    entry raised to 25 ... 60 above the rest of its row.  equal_row: every entry the same (uniform softmax, arg-max 0);
    argmax_row: the target is the dominant entry (loss below float32 epsilon); underflow_row: the target lies 150 below
    the maximum (its float32 probability is 0)."""
    x = LOGIT_SCALE * rng.standard_normal((rows, V))
    x += np.where(np.arange(rows) % 2 == 0, LOGIT_SHIFT, -LOGIT_SHIFT)[:, None]
    top = rng.integers(0, V, rows)
    x[np.arange(rows), top] = x.max(1) + rng.uniform(25, 60, rows)
    tg = rng.integers(0, V, rows) if targets is None else np.array(targets).reshape(rows)
    if equal_row is not None:
        x[equal_row] = x[equal_row, 0]
    if argmax_row is not None:
        tg[argmax_row] = top[argmax_row]
    if underflow_row is not None:
        tg[underflow_row] = (top[underflow_row] + 1) % V
        x[underflow_row, tg[underflow_row]] = x[underflow_row].max() - 150.0
    return x.astype(np.float32), tg.astype(np.int32)


def top1_lead(x):
    """largest minus second largest entry of every row"""
    s = np.sort(np.asarray(x, np.float64), -1)
    return s[..., -1] - s[..., -2]


def peaked_projection(W_o, b_o, h):
    """W_o scaled so that the logits h W_o spread like 30 N(0,1), and the shift + 200 in b_o (a projection cannot
    alternate the sign by row)"""
    lg = np.asarray(h, np.float64) @ np.asarray(W_o, np.float64)
    return (W_o * (LOGIT_SCALE / lg.std())).astype(np.float32), (np.asarray(b_o) + LOGIT_SHIFT).astype(np.float32)


# ------------------------------------------------------------------------------------------------- saturated ---------
def saturate(x, peak=PEAK):
    """x scaled so that max|x| = peak (float32)"""
    x = np.asarray(x, np.float64)
    return (x * (peak / np.abs(x).max())).astype(np.float32)


def saturate_partials(g, bias=None, peak=PEAK):
    """split-K partials g [S, ...] scaled so that their sum (+ bias) reaches +-peak"""
    tot = np.asarray(g, np.float64).sum(0)
    lo, hi = 0.0, 1e4
    for _ in range(60):                     # max|s tot + bias| = peak, monotone in s from max|bias| < peak on
        s = 0.5 * (lo + hi)
        lo, hi = (s, hi) if np.abs(s * tot + (0 if bias is None else bias)).max() < peak else (lo, s)
    return (np.asarray(g, np.float64) * hi).astype(np.float32)


# ------------------------------------------------------------------------------------------------- shortcuts ---------
F32 = np.float32


def one_pass_layer_norm(z, g, b, eps=1e-12):
    """LayerNorm with var = max(E[z^2] - E[z]^2, 0) in float32: -> y, xhat"""
    z, g, b = F32(z), F32(g), F32(b)
    n = F32(z.shape[-1])
    mean = z.sum(-1, keepdims=True, dtype=F32) / n
    var = np.maximum((z * z).sum(-1, keepdims=True, dtype=F32) / n - mean * mean, F32(0))
    rstd = F32(1) / np.sqrt(var + F32(eps))
    xhat = (z - mean) * rstd
    return xhat * g + b, xhat


def two_pass_layer_norm(z, g, b, eps=1e-12, dtype=np.float32):
    z, g, b = (np.asarray(a, dtype) for a in (z, g, b))
    mean = z.mean(-1, keepdims=True)
    var = ((z - mean) ** 2).mean(-1, keepdims=True)
    xhat = (z - mean) / np.sqrt(var + dtype(eps))
    return xhat * g + b, xhat


def softmax_no_max(x):
    with np.errstate(all='ignore'):
        e = np.exp(F32(x))
        return e / e.sum(-1, keepdims=True, dtype=F32)


def loss_from_probability(x, targets, dtype=np.float32):
    """-log(softmax(x)[target]): the softmax subtracts its maximum, the probability underflows all the same"""
    x = np.asarray(x, dtype)
    e = np.exp(x - x.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    with np.errstate(all='ignore'):
        return -np.log(np.take_along_axis(p, np.asarray(targets)[..., None], -1)[..., 0])


def tanh_exp_ratio(x):
    """(e^2x - 1) / (e^2x + 1) in float32: inf / inf above x = 44.4"""
    with np.errstate(all='ignore'):
        e = np.exp(F32(2) * F32(x))
        return (e - F32(1)) / (e + F32(1))


def lse_merge(x, chunk, guard=True, dtype=np.float32):
    """log-sum-exp of every row over chunks of `chunk` columns, merged as the streaming kernels do: each chunk gives
    (max, sum exp(x - max)); (m, s) + (pm, ps) -> (mx, s exp(m - mx) + ps exp(pm - mx)).  guard: a side whose maximum is -inf
    contributes nothing (without it, -inf - -inf is NaN)."""
    x = np.asarray(x, dtype)
    m = np.full(x.shape[:-1], -np.inf, dtype)
    s = np.zeros(x.shape[:-1], dtype)
    with np.errstate(all='ignore'):
        for lo in range(0, x.shape[-1], chunk):
            c = x[..., lo:lo + chunk]
            pm = c.max(-1)
            ps = np.exp(c - np.where(np.isinf(pm), dtype(0), pm)[..., None]).sum(-1, dtype=dtype) if guard else \
                np.exp(c - pm[..., None]).sum(-1, dtype=dtype)
            mx = np.maximum(m, pm)
            if guard:
                a = np.where(np.isinf(m) & (m < 0), dtype(0), np.exp(m - mx))
                b = np.where(np.isinf(pm) & (pm < 0), dtype(0), np.exp(pm - mx))
                ps = np.where(np.isinf(pm) & (pm < 0), dtype(0), ps)
            else:
                a, b = np.exp(m - mx), np.exp(pm - mx)
            s = s * a + ps * b
            m = mx
        return m + np.log(s)


def top_p_keep(x, p, dtype=np.float64):
    """nucleus of every row: tokens in descending order are kept while the mass BEFORE them is below p (the first token
    always).  float64: the reference; float32: cumulative sums that round, the shortcut an integer mass avoids."""
    x = np.asarray(x, dtype)
    order = np.argsort(-x, -1, kind='stable')
    xs = np.take_along_axis(x, order, -1)
    e = np.exp(xs - xs[..., :1])
    prob = e / e.sum(-1, keepdims=True, dtype=dtype)
    before = np.cumsum(prob, -1, dtype=dtype) - prob
    keep_sorted = before < dtype(p)
    keep = np.zeros(x.shape, bool)
    np.put_along_axis(keep, order, keep_sorted, -1)
    return keep
