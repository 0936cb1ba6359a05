"""The consensus (minimum-Bayes-risk) selector of include/comic_hip.h, comic_caption_consensus, restated in plain
Python / numpy float64: units, n-gram keys, the idf table and its builder, the CIDEr-D similarity, the utilities and the
choice.  Test infrastructure: the GPU tests compare the device operator against it, the CPU tests compare it against
oracle.scorer_ref.CiderD."""
import math

import numpy as np

N_ORDERS = 4
MASK64 = (1 << 64) - 1


def splitmix64(z):
    """csrc/splitmix.h on a numpy uint64 (scalar or array); wraps modulo 2^64."""
    with np.errstate(over='ignore'):
        z = np.uint64(z) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def ngram_key(tokens):
    """The 64-bit key of an n-gram given as its m = k * stride tokens in order; never 0."""
    h = splitmix64(len(tokens))
    for t in tokens:
        h = splitmix64(h ^ np.uint64(int(t)))
    return int(h) or 1


def build_table(entries, min_cap=1):
    """entries: {key: g}.  -> (keys uint64 [cap], g float64 [cap]): open addressing, linear probing from key & (cap - 1),
    cap the smallest power of two >= max(2 * len(entries), min_cap)."""
    cap = 1
    while cap < max(2 * len(entries), min_cap, 1):
        cap *= 2
    keys, g = np.zeros(cap, np.uint64), np.zeros(cap, np.float64)
    for key, val in entries.items():
        assert 0 < key <= MASK64
        at = key & (cap - 1)
        while keys[at] != 0:
            assert int(keys[at]) != key
            at = (at + 1) & (cap - 1)
        keys[at], g[at] = key, val
    return keys, g


def table_lookup(table, key, missing):
    keys, g = table
    cap = len(keys)
    at = key & (cap - 1)
    for _ in range(cap):
        if int(keys[at]) == key:
            return float(g[at])
        if keys[at] == 0:
            break
        at = (at + 1) & (cap - 1)
    return missing


def df_table(df, ref_len, stride=1, encode=None, min_cap=1):
    """A table from {tuple of words: document frequency}; encode maps a word to its token list (default: the word is
    its own single token id)."""
    entries = {}
    for ng, cnt in df.items():
        toks = [t for w in ng for t in (encode[w] if encode is not None else [w])]
        assert len(toks) == len(ng) * stride
        entries[ngram_key(toks)] = math.log(float(ref_len)) - math.log(max(1.0, float(cnt)))
    return build_table(entries, min_cap)


def units(row, end_id, stride):
    """The units of a candidate row: tuples of `stride` tokens in front of the first end_id, a partial last one dropped."""
    row = [int(x) for x in row]
    L = row.index(end_id) if end_id in row else len(row)
    return [tuple(row[i * stride:(i + 1) * stride]) for i in range(L // stride)]


def vectors(row, end_id, stride, table=None, log_ref_len=0.0):
    """-> (vec: per order a dict n-gram key -> tf * g in order of first occurrence, norm [4], len)."""
    u = units(row, end_id, stride)
    vec, norm = [], []
    for k in range(1, N_ORDERS + 1):
        tf = {}
        for i in range(len(u) - k + 1):
            key = ngram_key([t for unit in u[i:i + k] for t in unit])
            tf[key] = tf.get(key, 0) + 1
        v = {}
        for key, c in tf.items():
            g = 1.0 if table is None else table_lookup(table, key, log_ref_len)
            v[key] = float(c) * g
        vec.append(v)
        s = 0.0
        for x in v.values():
            s += x * x
        norm.append(math.sqrt(s))
    return vec, norm, max(len(u) - 1, 0)


def sim(h, r, sigma=6.0):
    """10 * mean over the orders of the CIDEr-D value of candidate h against sibling r (both from vectors())."""
    (vh, nh, lh), (vr, nr, lr) = h, r
    d = float(lh - lr)
    pen = math.exp(-(d * d) / (2.0 * sigma * sigma))
    total = 0.0
    for k in range(N_ORDERS):
        val = 0.0
        for key, w in vh[k].items():
            x = vr[k].get(key)
            if x is not None:
                val += min(w, x) * x
        if nh[k] != 0 and nr[k] != 0:
            val /= nh[k] * nr[k]
        total += val * pen
    return total / N_ORDERS * 10.0


def slot_weights(log_probs, W):
    """pi [W]: ones without log-probabilities, else their softmax in float64 (-inf -> 0; all -inf -> all 0)."""
    if log_probs is None:
        return np.ones(W)
    lp = np.asarray(log_probs, np.float32).astype(np.float64)
    m = lp.max()
    if not m > -np.inf:
        return np.zeros(W)
    e = np.array([math.exp(x - m) if x > -np.inf else 0.0 for x in lp])
    z = 0.0
    for x in e:
        z += x
    return e / z


def consensus(ids, end_id, stride=1, log_probs=None, table=None, log_ref_len=0.0, sigma=6.0):
    """ids [T, B, W] -> (utility [B, W] float64, best [B] int32).  log_probs [B, W] selects the 'posterior' mode."""
    ids = np.asarray(ids)
    T, B, W = ids.shape
    util, best = np.zeros((B, W)), np.zeros(B, np.int32)
    for b in range(B):
        cand = [vectors(ids[:, b, w], end_id, stride, table, log_ref_len) for w in range(W)]
        pi = slot_weights(None if log_probs is None else log_probs[b], W)
        for w in range(W):
            num = den = 0.0
            for j in range(W):
                if j != w:
                    num += pi[j] * sim(cand[w], cand[j], sigma)
                    den += pi[j]
            util[b, w] = -np.inf if not pi[w] > 0 else (num / den if den > 0 else 0.0)
        top, at = -np.inf, 0
        for w in range(W):
            if pi[w] > 0 and util[b, w] > top:
                top, at = util[b, w], w
        best[b] = at
    return util, best
