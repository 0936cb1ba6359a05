"""Reference of beam search with required words (banks by constraint progress) for the tests, in plain Python and numpy
float64: the progress of a history (progress), the per-step table a live row needs (base_and_specials), one banked step on
such a table (ref_select_banks), the inputs of the operator tests, and the ensemble reference loop of
tests/beam_constraints_ref.py with the banked initial state and selection (required_reference).

The rule (include/comic_hip.h, comic_beam_required): C words of S tokens per image (req [B,C,S], -1 rows = padding),
banks = C*S + 1, Wb = W / banks, slot w in bank w // Wb.  With k = L mod S, m = the words that are padding or have an aligned
full match in h, progress(h) = S*m + (k if some unmet word's first k tokens are h's tail else 0).  A candidate (w, v) goes to
bank progress(h_w ++ v) (live parent) or stays in w // Wb (finished parent); bank c takes its Wb best among the candidates of
all W parents with dest == c and a finite total, score descending then flat index w*V + v ascending; a slot without a
candidate is a dead slot (parent = itself, word = end_id, -inf, finished, its own previous length).

Margin rule: that of tests/test_gpu_ensemble.py (same GAP), per bank -- over the ranks 1 ... min(Wb, eligible) + 1 of the
bank's eligible list, consecutive float64 scores differ by more than GAP * max(1, |score|); margin is the smallest such
ratio over all entries and banks (inf where a bank has at most one eligible candidate), > 1 claims every id."""
import functools

import numpy as np

N_SPECIAL = 4


def _words(req_b):
    return [[int(x) for x in row] for row in np.asarray(req_b).reshape(len(req_b), -1)]


def _met(h, words, S):
    L = len(h)
    return [row[0] < 0 or any(h[i:i + S] == row for i in range(0, L - S + 1, S)) for row in words]


def progress(h, req_b, S):
    """progress(h) in [0, C*S] for the history h (a token list) under the words req_b [C,S]."""
    h = [int(x) for x in h]
    words = _words(req_b)
    met = _met(h, words, S)
    m, k = sum(met), len(h) % S
    partial = k > 0 and any(not met[q] and h[len(h) - k:] == words[q][:k] for q in range(len(words)))
    return S * m + (k if partial else 0)


def base_and_specials(h, req_b, S):
    """-> (base, special [4,2] int32 of (token, dest), token -1 = unused; slot q belongs to word q)."""
    h = [int(x) for x in h]
    words = _words(req_b)
    L, C = len(h), len(words)
    met = _met(h, words, S)
    m, k = sum(met), L % S
    lead = [not met[q] and h[L - k:] == words[q][:k] for q in range(C)]
    special = np.zeros((N_SPECIAL, 2), np.int32)
    special[:, 0] = -1
    for q in range(C):
        if not lead[q]:
            continue
        v = words[q][k]
        if k + 1 < S:
            dest = S * m + k + 1
        else:
            dest = S * (m + sum(1 for p in range(C) if lead[p] and words[p][k] == v))
        special[q] = (v, dest)
    return S * m, special


def table_dest(base, special, finished, V, banks):
    """dest [B,W,V] of every candidate: a finished parent's own bank, else base with the specials on top (the first special
    that names a token decides; tokens outside [0,V) are unused)."""
    B, W = np.asarray(base).shape
    Wb = W // banks
    dest = np.repeat(np.asarray(base, np.int64)[:, :, None], V, axis=2)
    for b in range(B):
        for w in range(W):
            if finished[b, w]:
                dest[b, w, :] = w // Wb
                continue
            for k in range(N_SPECIAL - 1, -1, -1):
                tok, d = int(special[b, w, k, 0]), int(special[b, w, k, 1])
                if 0 <= tok < V:
                    dest[b, w, tok] = d
    return dest


def ref_select_banks(lp, log_probs, finished, lengths, end_id, lpw, base, special, banks):
    """One banked step on the step distribution lp [B,W,V] (float64; -inf where a live beam is banned) and the table
    base [B,W], special [B,W,4,2].  -> dict(word, parent, scores, log_probs, finished, lengths, margin, eligible [B,banks])."""
    from tests.test_gpu_ensemble import F32_MIN, GAP
    B, W, V = lp.shape
    assert W % banks == 0
    Wb = W // banks
    lengths = np.asarray(lengths, np.int64)
    fin = np.asarray(finished, bool)
    fin_row = np.full(V, F32_MIN, np.float64)
    fin_row[end_id] = 0
    step = np.where(fin[:, :, None], fin_row[None, None, :], lp)
    with np.errstate(invalid='ignore'):
        total = np.asarray(log_probs, np.float64)[:, :, None] + step
    if lpw != 0:
        add = np.ones(V, np.int64)
        add[end_id] = 0
        new_len = lengths[:, :, None] + add[None, None, :] * (~fin)[:, :, None]
        score = total / ((5.0 + new_len) / 6.0) ** np.float64(np.float32(lpw))
    else:
        score = total
    dest = table_dest(base, special, fin, V, banks)
    ok = np.isfinite(total)
    word = np.full((B, W), end_id, np.int32)
    parent = np.tile(np.arange(W, dtype=np.int32), (B, 1))
    scores = np.full((B, W), -np.inf, np.float64)
    new_lp = np.full((B, W), -np.inf, np.float64)
    new_fin = np.ones((B, W), np.int32)
    new_len = lengths.copy()
    eligible = np.zeros((B, banks), np.int64)
    margin = np.inf
    for b in range(B):
        flat_s, flat_t, flat_d, flat_ok = (a[b].reshape(W * V) for a in (score, total, dest, ok))
        for c in range(banks):
            idx = np.nonzero((flat_d == c) & flat_ok)[0]                      # ascending flat index
            eligible[b, c] = len(idx)
            order = idx[np.argsort(-flat_s[idx], kind='stable')[:Wb + 1]]
            top = flat_s[order]
            if len(top) > 1:
                gaps = top[:-1] - top[1:]
                margin = min(margin, float((gaps / (GAP * np.maximum(1.0, np.abs(top[:-1])))).min()))
            for r, f in enumerate(order[:Wb]):
                o = c * Wb + r
                p, v = int(f) // V, int(f) % V
                word[b, o], parent[b, o], scores[b, o], new_lp[b, o] = v, p, flat_s[f], flat_t[f]
                new_fin[b, o] = int(fin[b, p] or v == end_id)
                new_len[b, o] = lengths[b, p] + (0 if fin[b, p] else 1)
    return dict(word=word, parent=parent, scores=scores, log_probs=new_lp, finished=new_fin, lengths=new_len, margin=margin,
                eligible=eligible)


def init_state(req, W, S):
    """Entry b's one live slot: the first slot of bank S * (its padding rows), log-probability 0."""
    req = np.asarray(req)
    B, C = req.shape[:2]
    Wb = W // (C * S + 1)
    log_probs = np.full((B, W), -np.inf, np.float32)
    finished = np.ones((B, W), np.int32)
    for b in range(B):
        w = S * int((req[b, :, 0] < 0).sum()) * Wb
        log_probs[b, w], finished[b, w] = 0, 0
    return log_probs, finished, np.zeros((B, W), np.int64)


def result_rule(last_scores, banks, S):
    """-> (best_slot [B], met [B]): the first slot of the highest bank whose first slot has a finite final score."""
    last_scores = np.asarray(last_scores)
    B, W = last_scores.shape
    Wb = W // banks
    best = np.zeros(B, np.int64)
    for b in range(B):
        ok = [c for c in range(banks) if np.isfinite(last_scores[b, c * Wb])]
        best[b] = (ok[-1] if ok else 0) * Wb
    return best, best // Wb // S


def table_of(hists, req, S, W):
    """The table of the rows with histories `hists` (a list of B*W token lists)."""
    R = len(hists)
    base = np.zeros(R, np.int32)
    special = np.zeros((R, N_SPECIAL, 2), np.int32)
    for r, h in enumerate(hists):
        base[r], special[r] = base_and_specials(h, req[r // W], S)
    return base.reshape(-1, W), special.reshape(-1, W, N_SPECIAL, 2)


# ------------------------------------------------------------------ inputs of the operator tests ---------------------------
def random_req(rng, B, C, S, V, pad_last=False):
    """A table of distinct tokens below V - 1 (end_id = V - 1); pad_last: the last word of entry 0 is padding."""
    req = rng.choice(V - 1, size=(B, C, S), replace=False).astype(np.int32) if B * C * S <= V - 1 else \
        rng.integers(0, V - 1, (B, C, S)).astype(np.int32)
    if pad_last and C > 1:
        req[0, C - 1, :] = -1
    return req


def history_of_progress(rng, req_b, S, c, V, n_words=2):
    """A history of n_words * S + (c % S) tokens whose progress is c: c // S required words (the first unmet ones), filler
    words that match nothing, then the first c % S tokens of the next unmet word."""
    words = [w for w in _words(req_b) if w[0] >= 0]
    pad = len(req_b) - len(words)
    m, k = c // S - pad, c % S
    assert 0 <= m <= len(words) and (k == 0 or m < len(words))
    used = {t for w in words for t in w}

    def filler():
        out = []
        while len(out) < S:
            t = int(rng.integers(0, V - 1))
            if t not in used:
                out.append(t)
        return out
    h = []
    for j in range(max(n_words, m)):
        h += words[j] if j < m else filler()
    if k:
        h += words[m][:k]
    assert progress(h, req_b, S) == c, (h, req_b, c)
    return h


@functools.lru_cache(maxsize=None)
def banks_inputs(shape, C, S, state, seed=0, table='rule'):
    """logits / weights as tests/test_gpu_ensemble.step_case, a table req [B,C,S], and a state.
    init: the initial state (every history empty).  mid: slot w of every entry holds a history of progress w // Wb (a bank
    whose progress the entry's padding makes unreachable holds dead slots: finished, -inf), one live slot per entry finished
    with its log-probability kept, log-probabilities and lengths random.
    table='rule': the table of the histories.  table='random': bases anywhere at or below the row's own bank and up to four
    specials per row that lead into any bank (distinct tokens).  table='low': every base 0 and no finished beam (bank 0 scans every row that holds one)."""
    n, B, W, V = shape
    banks = C * S + 1
    Wb = W // banks
    rng = np.random.default_rng(seed)
    logits = (2.0 * rng.standard_normal((n, B, W, V))).astype(np.float32)
    wts = np.ones(1, np.float32) if n == 1 else rng.dirichlet(np.ones(n)).astype(np.float32)
    end_id = V - 1
    req = random_req(rng, B, C, S, V, pad_last=True)
    if state == 'init':
        log_probs, finished, lengths = init_state(req, W, S)
        hists = [[] for _ in range(B * W)]
    else:
        log_probs = -rng.uniform(1.0, 6.0, (B, W)).astype(np.float32)
        finished = np.zeros((B, W), np.int32)
        lengths = rng.integers(1, 7, (B, W)).astype(np.int64)
        hists = []
        for b in range(B):
            pad = int((req[b, :, 0] < 0).sum())
            for w in range(W):
                c = w // Wb
                if c < S * pad:                               # unreachable: a dead slot
                    hists.append([end_id])
                    log_probs[b, w], finished[b, w] = -np.inf, 1
                else:
                    hists.append(history_of_progress(rng, req[b], S, c, V))
            live = [w for w in range(W) if not finished[b, w]]
            finished[b, live[int(rng.integers(0, len(live)))]] = 1
    base, special = table_of(hists, req, S, W)
    if table == 'low':
        finished = np.where(np.isfinite(log_probs), 0, finished).astype(np.int32)      # every slot that holds a beam is live
    if table != 'rule':
        own = np.arange(W)[None, :] // Wb
        base = (rng.integers(0, banks, (B, W)) % (own + 1)).astype(np.int32) if table == 'random' else np.zeros((B, W), np.int32)
        special = np.zeros((B, W, N_SPECIAL, 2), np.int32)
        for b in range(B):
            for w in range(W):
                special[b, w, :, 0] = rng.choice(V - 1, N_SPECIAL, replace=False)
                special[b, w, :, 1] = rng.integers(0, banks, N_SPECIAL)
                special[b, w, int(rng.integers(0, N_SPECIAL)), 0] = -1
    return dict(logits=logits, wts=wts, end_id=end_id, log_probs=log_probs, finished=finished, lengths=lengths, req=req,
                base=base, special=special, banks=banks, hists=hists)


@functools.lru_cache(maxsize=None)
def banks_case(shape, C, S, state, lpw, seed=0, table='rule'):
    """banks_inputs + the float64 reference (`ref`) and the unbanked reference of the same state (`plain`)."""
    from tests.test_gpu_ensemble import ref_select, ref_step_lp
    c = dict(banks_inputs(shape, C, S, state, seed, table))
    c['lp'] = ref_step_lp(c['logits'], c['wts'])
    c['ref'] = ref_select_banks(c['lp'], c['log_probs'], c['finished'], c['lengths'], c['end_id'], lpw, c['base'],
                                c['special'], c['banks'])
    c['plain'] = ref_select(c['lp'], c['log_probs'], c['finished'], c['lengths'], c['end_id'], lpw)
    return c


# ------------------------------------------------------------------ the whole decoder ---------------------------------------
def required_reference(members, wts, fm, im, W, max_steps, req, S, **cons):
    """constrained_reference of tests/beam_constraints_ref.py with the banked initial state and selection (cons empty: no
    bans).  -> step_ids, parent_ids, scores [T,B,W], lengths, log_probs [B,W] (the final state), margin, hists (the final
    histories, B*W token lists), banks, best_slot, met."""
    from oracle import decoder_ref as dr
    from tests.beam_constraints_ref import ban_mask
    from tests.test_gpu_ensemble import ref_step_lp
    req = np.asarray(req, np.int32)
    B, C = fm.shape[0], req.shape[1]
    banks = C * S + 1
    cfg0 = members[0][1]
    V = cfg0.softmax_size
    st = []
    for p, cfg in members:
        keys, values = dr.memory_projections(p, cfg, np.repeat(fm, W, axis=0))
        c, h, _ = dr.rnn_init(p, cfg, np.repeat(im, W, axis=0), None)
        st.append(dict(keys=keys, values=values, c=c, h=h, att=np.zeros((B * W, cfg.attn_size), np.float32)))
    log_probs, finished, lengths = init_state(req, W, S)
    log_probs = log_probs.astype(np.float64)
    ids = np.full(B * W, cfg0.start_id, np.int64)
    hists = [[] for _ in range(B * W)]
    out = dict(step_ids=[], parent_ids=[], scores=[])
    margin = np.inf
    for t in range(max_steps):
        logits = []
        for (p, cfg), s in zip(members, st):
            y, s['c'], s['h'], s['att'], _, _ = dr.decoder_step(p, cfg, s['keys'], s['values'], dr.embed(p['emb'], ids),
                                                                s['c'], s['h'], s['att'], None)
            logits.append((y @ p['W_o'] + p['b_o']).reshape(B, W, V))
        lp = ref_step_lp(np.stack(logits), wts)
        if cons:
            mask = ban_mask(hists, finished.reshape(-1), lengths.reshape(-1), V, cfg0.end_id, **cons).reshape(B, W, V)
            lp = np.where(mask, -np.inf, lp)
        base, special = table_of(hists, req, S, W)
        r = ref_select_banks(lp, log_probs, finished, lengths, cfg0.end_id, 0.0, base, special, banks)
        margin = min(margin, r['margin'])
        log_probs, finished, lengths = r['log_probs'], r['finished'], r['lengths']
        gidx = (np.arange(B)[:, None] * W + r['parent']).reshape(-1)
        for s in st:
            s['c'], s['h'], s['att'] = s['c'][gidx], s['h'][gidx], s['att'][gidx]
        hists = [hists[g] + [int(w)] for g, w in zip(gidx, r['word'].reshape(-1))]
        out['step_ids'].append(r['word']); out['parent_ids'].append(r['parent']); out['scores'].append(r['scores'])
        ids = r['word'].reshape(-1).astype(np.int64)
        if finished.all():
            break
    res = {k: np.stack(v) for k, v in out.items()}
    best, met = result_rule(res['scores'][-1], banks, S)
    res.update(lengths=lengths, log_probs=log_probs, margin=float(margin), hists=hists, banks=banks, best_slot=best, met=met)
    return res
