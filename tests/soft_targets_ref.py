"""Soft-target XE training (include/comic_hip.h, comic_soft_targets / comic_teacher_topk) restated in float64 numpy, and
the shared operand builders of tests/test_soft_targets_cpu.py and tests/test_gpu_soft_targets.py (fixed seeds: both sides
build the same arrays).

The loss rule, for a live row with logits z, p = softmax(z), target y, eps = smoothing, lam = teacher_weight:
    q_T(v) = sum_k [ids_k = v] probs_k / sum_k probs_k
    q      = (1 - eps - lam) e_y + eps / V + lam q_T
    loss   = wmask (lse(z) - sum_v q_v z_v)         (cross-entropy H(q, p))
    nll    = wmask (lse(z) - z_y)
    dl     = (p - q) coef
The table rule, for n members with weights w and temperature tau:
    pbar = sum_m w_m softmax(z_m / tau); the K largest, ordered by (pbar descending, id ascending)."""
import numpy as np

from oracle import decoder_ref as dr
from tests import regimes

GAP_MIN = 1e-5          # smallest relative gap between consecutive ranks 1 .. K+1 the exact-id comparison allows


def f64(x):
    return np.asarray(x, np.float64)


def teacher_q(ids, probs, V):
    """Dense q_T [..., V] of a table ids / probs [..., K]; rows with sum(probs) == 0 give zeros."""
    ids, probs = np.asarray(ids), f64(probs)
    S = probs.sum(-1, keepdims=True)
    q = np.zeros(ids.shape[:-1] + (V,))
    np.put_along_axis(q, ids.astype(np.int64), np.divide(probs, S, out=np.zeros_like(probs), where=S > 0), -1)
    return q


def soft_target(targets, V, eps, lam, ids=None, probs=None):
    """q [..., V] for integer targets [...]"""
    oh = np.zeros(np.shape(targets) + (V,))
    np.put_along_axis(oh, np.asarray(targets, np.int64)[..., None], 1.0, -1)
    q = (1.0 - eps - lam) * oh + eps / V
    if lam:
        q = q + lam * teacher_q(ids, probs, V)
    return q


def soft_xent_ref(logits, targets_bt, coef_bt, wmask_bt, lens, eps, lam, ids=None, probs=None):
    """Time-major logits [T,B,V] against [B,Ts] tables (Ts >= T) and a table [T,B,K], as tests.exec_ops_ref.xent_ref:
    -> dict(logits (finished rows zeroed), loss [T,B], nll [T,B], dlogits [T,B,V], ids [T,B], q [T,B,V])."""
    T, B, V = logits.shape
    live = np.arange(T)[:, None] < np.asarray(lens)[None, :]
    lg = logits * live[..., None]
    z = f64(lg)
    lsm = dr.log_softmax(z, -1)
    tg = np.asarray(targets_bt)[:, :T].T
    q = soft_target(tg, V, eps, lam, ids, probs)
    w, c = f64(wmask_bt)[:, :T].T, f64(coef_bt)[:, :T].T
    loss = -(q * lsm).sum(-1) * w * live
    nll = -np.take_along_axis(lsm, tg[..., None].astype(np.int64), 2)[..., 0] * w * live
    dl = (np.exp(lsm) - q) * c[..., None] * live[..., None]
    return dict(logits=lg, loss=loss, nll=nll, dlogits=dl, ids=lg.argmax(-1) * live, q=q)


def mean_probability(logits, weights, tau):
    """pbar [..., V] of members' logits [n][..., V]"""
    return sum(float(w) * np.exp(dr.log_softmax(f64(z) / float(tau), -1)) for z, w in zip(logits, weights))


def topk_rule(p, K):
    """ids, values [..., K] of the K largest entries of p [..., V] by (value descending, id ascending)"""
    order = np.argsort(-f64(p), axis=-1, kind='stable')[..., :K]       # stable: equal values keep their id order
    return order.astype(np.int32), np.take_along_axis(f64(p), order, -1)


def teacher_topk_ref(logits, weights, lens, Tp, tau, K):
    """-> ids [T,B,K] int32, probs [T,B,K], pbar [T,B,V]; rows with t >= Tp or t >= lens[b]: ids 0 .. K-1, probs 0."""
    T, B, V = np.shape(logits[0])
    pbar = mean_probability(logits, weights, tau)
    ids, probs = topk_rule(pbar, K)
    live = (np.arange(T)[:, None] < np.asarray(lens)[None, :]) & (np.arange(T)[:, None] < Tp)
    ids = np.where(live[..., None], ids, np.arange(K, dtype=np.int32))
    return ids.astype(np.int32), probs * live[..., None], pbar


def rank_gaps(pbar, K):
    """smallest relative gap (p_i - p_{i+1}) / p_i between consecutive ranks 1 .. K+1 of every row (1 .. V when K = V)"""
    s = -np.sort(-f64(pbar), -1)[..., :K + 1]
    return ((s[..., :-1] - s[..., 1:]) / s[..., :-1]).min(-1)


# ------------------------------------------------------------------------------------------- shared operand builders --
B, T_ROWS, T_STRIDE = 3, 3, 4           # one batch row ends before t_rows, one token has wmask 0
LENS = np.array([3, 2, 4], np.int32)
V_CASES = (258, 4099)                   # 4099: not a multiple of 256
K_CASES = (1, 8)
SETTINGS = ((0.1, 0.0), (0.0, 1.0), (0.1, 0.5))
TEACHER_CASES = [(V, K, n, tau) for V in V_CASES for K in K_CASES for n, tau in ((1, 1.0), (3, 2.0), (3, 1.0), (1, 2.0))]
WEIGHTS = {1: (1.0,), 3: (0.5, 0.3, 0.2)}


def teacher_logits(V, n, seed=0):
    """n members' logits [T_STRIDE,B,V] float32, N(0,1) * 3.  (The seeds are chosen for the input condition of the exact-id
    comparison, rank_gaps > GAP_MIN on every row -- tests/test_soft_targets_cpu.py holds it; the smallest gap is 1.1e-4.)"""
    rng = np.random.default_rng(2000 + 7 * V + n + seed)
    return [(3 * rng.standard_normal((T_STRIDE, B, V))).astype(np.float32) for _ in range(n)]


def xent_case(V, K, regime=None):
    """Operands of the soft loss: logits [T_ROWS,B,V], lens, targets [B,T_STRIDE], wmask, coef and a teacher table
    [T_STRIDE,B,K] built by the rule above from N(0,1) * 3 teacher logits that are raised at the target where t + b is even
    (the target is the table's first id) and lowered where it is odd (the target is outside the table)."""
    rng = np.random.default_rng(50 + V + K + (1 if regime else 0))
    if regime is None:
        logits = (3 * rng.standard_normal((T_ROWS, B, V))).astype(np.float32)
        targets = rng.integers(0, V, (B, T_STRIDE)).astype(np.int32)
    else:
        assert regime == 'peaked', regime
        lg, tg = regimes.peaked_logits(rng, T_ROWS * B, V, equal_row=0, argmax_row=B, underflow_row=2 * B)
        logits = lg.reshape(T_ROWS, B, V)
        targets = rng.integers(0, V, (B, T_STRIDE)).astype(np.int32)
        targets[:, :T_ROWS] = tg.reshape(T_ROWS, B).T
    wmask = (np.arange(T_STRIDE)[None, :] < LENS[:, None]).astype(np.float32)
    wmask[2, 1] = 0.0                                      # a live token without weight
    coef = (wmask / wmask.sum()).astype(np.float32)
    zt = teacher_logits(V, 1, seed=K)[0]
    even = (np.arange(T_STRIDE)[:, None] + np.arange(B)[None, :]) % 2 == 0
    np.put_along_axis(zt, targets.T[..., None].astype(np.int64), np.where(even, 40.0, -40.0)[..., None].astype(np.float32), 2)
    ids, probs, _ = teacher_topk_ref([zt], (1.0,), LENS, T_STRIDE, 1.0, K)
    inside = (ids == targets.T[..., None]).any(-1)
    live = np.arange(T_STRIDE)[:, None] < LENS[None, :]
    assert (inside == even)[live].all()
    return dict(logits=logits, lens=LENS.copy(), targets=targets, wmask=wmask, coef=coef, t_ids=ids,
                t_probs=probs.astype(np.float32))
