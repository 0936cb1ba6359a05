"""numpy / float64 restatement of the device SCST reward (comic_scst_reward, comic_scst_coefficients) on WORD IDS:
canonical words, n-gram keys, CIDEr-D, per-sentence BLEU-1..4, reward, baselines, advantage and the loss coefficients.

Test infrastructure: tests/test_scst_reward_cpu.py pins it to oracle/scorer_ref.py on text; tests/test_gpu_scst_reward.py
holds the kernels to it.  The sums run in the order oracle/scorer_ref.py forms them (n-grams in order of first
occurrence, references ascending)."""
from __future__ import annotations

import math

import numpy as np

NONE, ROW, LEAVE_ONE_OUT = 0, 1, 2          # COMIC_SCST_BASELINE_*


# ------------------------------------------------------------------ canonical words --
def canonical_words(row, token_type, end_id, n_ids, base=0, word_len=1):
    """One rollout's token ids -> the word ids ops.id_to_caption(skip_unmapped=True) turns into text.
    n_ids: the number of word ids the table maps (RewardVocab.n_ids)."""
    row = [int(t) for t in row]
    if token_type == 'word':
        return [t for t in row if 0 <= t < n_ids and t != end_id]
    digits = [t for t in row if 0 <= t < base]
    if len(digits) % word_len:               # ONE trailing digit, whatever the remainder
        digits = digits[:-1]
    words = []
    for i in range(0, len(digits), word_len):    # a short last group (word_len > 2) decodes as it stands
        v = 0
        for d in digits[i:i + word_len]:
            v = v * base + d
        words.append(v)
    return [w for w in words if w < n_ids]


# ----------------------------------------------------------------------------- keys --
_M = (1 << 64) - 1


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def ngram_key(words):
    """The 64-bit key of an n-gram of word ids (csrc/ngram_dev.h; one token per word)."""
    h = splitmix64(len(words))
    for w in words:
        h = splitmix64(h ^ (int(w) & _M))
    return h or 1


def cook(words, n=4):
    """{tuple of word ids: count}, in order of first occurrence, order 1 first (precook)."""
    counts = {}
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            ng = tuple(words[i:i + k])
            counts[ng] = counts.get(ng, 0) + 1
    return counts


# -------------------------------------------------------------------------- CIDEr-D --
def _vec(counts, df, log_ref_len, n=4):
    vec = [dict() for _ in range(n)]
    norm = [0.0] * n
    length = 0
    for ng, tf in counts.items():
        g = 1.0 if df is None else log_ref_len - math.log(max(1.0, float(df.get(ng, 0.0))))
        k = len(ng) - 1
        vec[k][ng] = float(tf) * g
        norm[k] += vec[k][ng] ** 2
        if k == 1:                           # the host scorer's quirk: length = number of bigrams
            length += tf
    return vec, [math.sqrt(x) for x in norm], length


def cider_d(hypo, refs, df, log_ref_len, sigma=6.0, n=4):
    """hypo: word ids; refs: list of word-id lists; df: {tuple of word ids: document count} or None (g = 1)."""
    vh, nh, lh = _vec(cook(hypo, n), df, log_ref_len, n)
    score = [0.0] * n
    for r in refs:
        vr, nr, lr = _vec(cook(r, n), df, log_ref_len, n)
        delta = float(lh - lr)
        for k in range(n):
            val = 0.0
            for ng, w in vh[k].items():
                x = vr[k].get(ng, 0.0)
                val += min(w, x) * x
            if nh[k] != 0 and nr[k] != 0:
                val /= nh[k] * nr[k]
            score[k] += val * math.exp(-(delta ** 2) / (2 * sigma ** 2))
    return (score[0] + score[1] + score[2] + score[3]) / n / len(refs) * 10.0


# ----------------------------------------------------------------------------- BLEU --
def bleu(hypo, refs, n=4):
    small, tiny = 1e-9, 1e-15
    maxcounts = {}
    for r in refs:
        for ng, c in cook(r, n).items():
            maxcounts[ng] = max(maxcounts.get(ng, 0), c)
    testlen = len(hypo)
    reflen = min((abs(len(r) - testlen), len(r)) for r in refs)[1]      # 'closest', ties to the shorter
    correct = [0] * n
    for ng, c in cook(hypo, n).items():
        correct[len(ng) - 1] += min(maxcounts.get(ng, 0), c)
    out, run = [], 1.0
    for k in range(n):
        run *= (float(correct[k]) + tiny) / (float(max(0, testlen - k)) + small)
        out.append(run ** (1.0 / (k + 1)))
    ratio = (testlen + tiny) / (reflen + small)
    if ratio < 1:
        out = [b * math.exp(1 - 1 / ratio) for b in out]
    return out


# --------------------------------------------------------------------------- reward --
def score(cands, refs, df, ref_len, w_cider, w_bleu, mode, has_row, sigma=6.0):
    """cands: [B][W'] word-id lists, the baseline row (has_row) last; refs: [B][R_b] word-id lists; df: {tuple of word
    ids: count} or None; mode: NONE / ROW / LEAVE_ONE_OUT.  -> dict(cider [B,W'], bleu [B,W',4], reward [B,W'],
    baseline [B,W] float64, advantage [W,B] float32)."""
    B, Wt = len(cands), len(cands[0])
    W = Wt - (1 if has_row else 0)
    log_ref_len = math.log(float(ref_len)) if df is not None else 0.0
    do_c, do_b = w_cider > 0, max(w_bleu) > 0
    cider, bl, rew = np.zeros((B, Wt)), np.zeros((B, Wt, 4)), np.zeros((B, Wt))
    for b in range(B):
        for h in range(Wt):
            total = 0.0
            if do_c:
                cider[b, h] = cider_d(cands[b][h], refs[b], df, log_ref_len, sigma)
                total += cider[b, h] * w_cider
            if do_b:
                bl[b, h] = bleu(cands[b][h], refs[b])
                for k in range(4):
                    total += bl[b, h, k] * w_bleu[k]
            rew[b, h] = total
    base = np.zeros((B, W))
    for b in range(B):
        for i in range(W):
            if mode == ROW:
                base[b, i] = rew[b, W]
            elif mode == LEAVE_ONE_OUT:
                s = 0.0
                for j in range(W):
                    if j != i:
                        s += rew[b, j]
                base[b, i] = s / (W - 1)
    adv = (rew[:, :W] - base).astype(np.float32).T.copy()
    return dict(cider=cider, bleu=bl, reward=rew, baseline=base, advantage=adv)


def score_ids(ids, refs, vocab, df, ref_len, w_cider, w_bleu, mode, baseline_ids=None, sigma=6.0, baseline_first_eos=None):
    """The operator's contract on raw ids: ids [T,B,W], baseline_ids [T0,B] or None, refs [B][R_b] word-id lists, vocab a
    decoder.RewardVocab (or anything with token_type, end_id, n_ids, radix_base, word_len)."""
    ids = np.asarray(ids)
    T, B, W = ids.shape
    canon = lambda row: canonical_words(row, vocab.token_type, vocab.end_id, vocab.n_ids, vocab.radix_base, vocab.word_len)
    cands = [[canon(ids[:, b, w]) for w in range(W)] for b in range(B)]
    if baseline_ids is not None:
        base = np.asarray(baseline_ids)
        if baseline_first_eos is not None:       # the rows the greedy loop executed: it ends when every image has its <EOS>
            base = base[:max(0, min(base.shape[0], int(np.max(baseline_first_eos)) + 1))]
        for b in range(B):
            cands[b].append(canon(base[:, b]))
    return score(cands, refs, df, ref_len, w_cider, w_bleu, mode, baseline_ids is not None, sigma)


# --------------------------------------------------------------------- coefficients --
def coefficients(wmask, adv):
    """Decoder.train_step's host formula in float32: -> (coef [B',T], rs [B',T])."""
    wmask = np.asarray(wmask, np.float32)
    Bp, T = wmask.shape
    den = wmask.sum(axis=1, keepdims=True) + np.float32(1e-12)
    rb = np.asarray(adv, np.float32)[:, None] / np.float32(Bp)
    rs = np.broadcast_to(rb / den, (Bp, T)).astype(np.float32)
    coef = wmask / den * rb
    return coef, rs
