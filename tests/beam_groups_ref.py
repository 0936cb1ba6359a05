"""Reference of diverse beam search (beam groups with a Hamming diversity penalty) for the tests, in numpy float64: one
step (ref_select_groups), the inputs that make groups collide (groups_case), and the ensemble reference loop of
tests/test_gpu_ensemble.py / tests/beam_constraints_ref.py with the grouped selection (diverse_reference).

The rule (include/comic_hip.h, comic_beam_groups): W slots in G groups of Wg = W / G, group g owning the slots
[g*Wg, (g+1)*Wg).  total = log_probs + step and score (total, or total / ((5 + len) / 6)^lpw) are the plain step's.  The
groups are decided in order; group g ranks candidate (w, v) by score - lam * count[v] when beam w is live and v is not
<EOS>, by score otherwise, count[v] being the number of slots q < g*Wg whose word chosen at this step is v; it takes its Wg
best among its own Wg * V candidates (rank descending, flat index w*V + v ascending).  `scores` is the rank, the state the
unpenalised total.

Margin rule: that of the two files above, per group -- in every entry and every group the float64 ranks 1 ... Wg + 1 of the
PENALISED ranking differ by more than GAP * max(1, |rank|); margin is the smallest such ratio, > 1 claims every id."""
import functools

import numpy as np

from tests.test_gpu_ensemble import F32_MIN, GAP, ref_step_lp


def ref_select_groups(lp, log_probs, finished, lengths, end_id, lpw, G, lam):
    """One grouped step on the step distribution lp [B,W,V] (float64; -inf where a live beam is banned).
    -> dict(word, parent, scores, log_probs, finished, lengths, margin) as tests/test_gpu_ensemble.ref_select."""
    B, W, V = lp.shape
    assert G >= 1 and W % G == 0
    Wg = W // G
    lengths = np.asarray(lengths, np.int64)
    fin = np.asarray(finished, bool)
    fin_row = np.full(V, F32_MIN, np.float64)
    fin_row[end_id] = 0
    step = np.where(fin[:, :, None], fin_row[None, None, :], lp)
    total = np.asarray(log_probs, np.float64)[:, :, None] + step
    if lpw != 0:
        add = np.ones(V, np.int64)
        add[end_id] = 0
        new_len = lengths[:, :, None] + add[None, None, :] * (~fin)[:, :, None]
        score = total / ((5.0 + new_len) / 6.0) ** np.float64(np.float32(lpw))
    else:
        score = total
    word = np.zeros((B, W), np.int32)
    parent = np.zeros((B, W), np.int32)
    scores = np.zeros((B, W), np.float64)
    new_lp = np.zeros((B, W), np.float64)
    margin = np.inf
    bidx = np.arange(B)[:, None]
    for g in range(G):
        w0 = g * Wg
        count = np.zeros((B, V), np.float32)
        for q in range(w0):
            count[np.arange(B), word[:, q]] += 1
        pen = (np.float32(lam) * count).astype(np.float64)                 # the fp32 product, subtracted once
        sub = pen[:, None, :] * (~fin[:, w0:w0 + Wg, None])                 # live beams only
        sub[:, :, end_id] = 0                                              # <EOS> is never penalised
        rank = np.where(sub != 0, score[:, w0:w0 + Wg] - sub, score[:, w0:w0 + Wg])
        flat = rank.reshape(B, Wg * V)
        order = np.argsort(-flat, axis=1, kind='stable')[:, :Wg + 1]
        top = np.take_along_axis(flat, order, axis=1)
        gaps = top[:, :-1] - top[:, 1:]
        margin = min(margin, float((gaps / (GAP * np.maximum(1.0, np.abs(top[:, :-1])))).min()))
        order = order[:, :Wg]
        word[:, w0:w0 + Wg] = order % V
        parent[:, w0:w0 + Wg] = w0 + order // V                            # entry-wide slots
        scores[:, w0:w0 + Wg] = top[:, :Wg]
        new_lp[:, w0:w0 + Wg] = total[bidx, parent[:, w0:w0 + Wg], word[:, w0:w0 + Wg]]
    prev_fin = fin[bidx, parent]
    return dict(word=word, parent=parent, scores=scores, log_probs=new_lp,
                finished=(prev_fin | (word == end_id)).astype(np.int32),
                lengths=lengths[bidx, parent] + (~prev_fin).astype(np.int64), margin=margin)


def init_state(B, W, G):
    """The first slot of each group live with log-probability 0, the others finished with -inf."""
    Wg = W // G
    log_probs = np.full((B, W), -np.inf, np.float32)
    log_probs[:, ::Wg] = 0
    finished = np.ones((B, W), np.int32)
    finished[:, ::Wg] = 0
    return log_probs, finished, np.zeros((B, W), np.int64)


@functools.lru_cache(maxsize=None)
def groups_inputs(shape, G, state, seed=0):
    """Inputs under which groups collide (independent random rows almost never do): the beams of an entry share a strong
    component, logits[m,b,w,:] = 2 N(0,1) [m,b,1,V] + 0.3 N(0,1) [m,b,w,V], drawn in that order; then the Dirichlet weights
    for n > 1; then the `mid` state exactly as tests/test_gpu_ensemble.step_case draws it."""
    n, B, W, V = shape
    rng = np.random.default_rng(seed)
    shared = rng.standard_normal((n, B, 1, V))
    own = rng.standard_normal((n, B, W, V))
    logits = (2.0 * shared + 0.3 * own).astype(np.float32)
    wts = np.ones(1, np.float32) if n == 1 else rng.dirichlet(np.ones(n)).astype(np.float32)
    end_id = V - 1
    if state == 'init':
        log_probs, finished, lengths = init_state(B, W, G)
    else:                                   # mid-decode: one finished beam per entry
        log_probs = -rng.uniform(1.0, 6.0, (B, W)).astype(np.float32)
        finished = np.zeros((B, W), np.int32)
        finished[np.arange(B), rng.integers(0, W, B)] = 1
        lengths = rng.integers(1, 7, (B, W)).astype(np.int64)
    return dict(logits=logits, wts=wts, end_id=end_id, log_probs=log_probs, finished=finished, lengths=lengths)


@functools.lru_cache(maxsize=None)
def groups_case(shape, G, state, lpw, lam=0.5, seed=0):
    """groups_inputs + the float64 reference at lam (`ref`) and at 0 (`ref0`), computed once and shared."""
    c = dict(groups_inputs(shape, G, state, seed))
    lp = ref_step_lp(c['logits'], c['wts'])
    c['lp'] = lp
    c['ref'] = ref_select_groups(lp, c['log_probs'], c['finished'], c['lengths'], c['end_id'], lpw, G, lam)
    c['ref0'] = ref_select_groups(lp, c['log_probs'], c['finished'], c['lengths'], c['end_id'], lpw, G, 0.0)
    return c


def diverse_reference(members, wts, fm, im, W, max_steps, G, lam, **cons):
    """constrained_reference of tests/beam_constraints_ref.py with the grouped initial state and selection (cons empty: no
    bans).  -> step_ids, parent_ids, scores [T,B,W], lengths, log_probs [B,W] (the final state), margin."""
    from oracle import decoder_ref as dr
    from tests.beam_constraints_ref import ban_mask
    B = fm.shape[0]
    cfg0 = members[0][1]
    V = cfg0.softmax_size
    st = []
    for p, cfg in members:
        keys, values = dr.memory_projections(p, cfg, np.repeat(fm, W, axis=0))
        c, h, _ = dr.rnn_init(p, cfg, np.repeat(im, W, axis=0), None)
        st.append(dict(keys=keys, values=values, c=c, h=h, att=np.zeros((B * W, cfg.attn_size), np.float32)))
    log_probs, finished, lengths = init_state(B, W, G)
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
        r = ref_select_groups(lp, log_probs, finished, lengths, cfg0.end_id, 0.0, G, lam)
        margin = min(margin, r['margin'])
        if cons:
            assert not mask[np.arange(B)[:, None], r['parent'], r['word']].any(), 'the reference selected a banned token'
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
    res.update(lengths=lengths, log_probs=log_probs, margin=float(margin))
    return res
