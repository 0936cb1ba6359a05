"""Reference of forced-prefix decoding for the tests: the forcing rule as a plain function over masks, and ONE float64
decode loop over the selections of the plain, grouped, sampled and banked reference loops with that rule applied after
the constraints' mask.

The rule (include/comic_hip.h, comic_beam_prefix): pfx [B, P] int32, -1 padded at the end of each row.  At step t row
(b, w) is forced when t < P, 0 <= pfx[b][t] < V and the row is live: its mask has every bit below V set except that
token's, replacing the constraints' mask.  A finished row bans nothing; any other row keeps the constraints' mask (all
False without constraints)."""
import numpy as np

from tests.beam_constraints_ref import ban_mask


def prefix_lengths(pfx):
    pfx = np.asarray(pfx)
    pad = pfx < 0
    return np.where(pad.any(axis=1), pad.argmax(axis=1), pfx.shape[1])


def forced_rows(pfx, finished, t, W, V):
    """-> (forced bool [R], token int [R]) of step t for the R = B * W rows."""
    pfx = np.asarray(pfx)
    B, P = pfx.shape
    tok = np.repeat(pfx[:, t] if t < P else np.full(B, -1, np.int64), W).astype(np.int64)
    forced = (tok >= 0) & (tok < V) & (np.asarray(finished).reshape(-1) == 0)
    return forced, tok


def forced_mask(mask, pfx, finished, t, W):
    """The rule on the constraints' mask (bool [R, V]; all False for no constraints) -> bool [R, V]."""
    R, V = mask.shape
    out = np.array(mask, bool)
    forced, tok = forced_rows(pfx, finished, t, W, V)
    fin = np.asarray(finished).reshape(-1) != 0
    out[fin] = False
    for r in np.nonzero(forced)[0]:
        out[r] = True
        out[r, tok[r]] = False
    return out


def _sub(a, keep):
    return None if a is None else np.asarray(a)[keep]


def prefixed_reference(members, wts, fm, im, W, max_steps, pfx, policy='beam', G=1, lam=0.0, seed=0, temperature=1.0,
                       image_base=0, req=None, S=1, top_k=0, top_p=1.0, **cons):
    """The reference loops of tests/beam_constraints_ref.py (policy 'beam'), tests/beam_groups_ref.py ('groups': G, lam),
    tests/beam_sampling_ref.py ('samples': seed, temperature, image_base) and tests/beam_required_ref.py ('banks': req, S)
    with the forced mask applied after the constraints' (cons empty: none).  members: [(params, cfg)].
    top_k / top_p ('samples' only): the truncation of tests/beam_truncate_ref.py after the forced mask.  Its rule is a
    sandwich (must_keep, must_drop and a band between them that fp32 may decide either way), so every step selects twice,
    once through the smallest mask the sandwich allows (only must_drop banned) and once through the largest (all but
    must_keep banned); `sandwich_agrees` says that both gave the same ids at every step, i.e. that no token of a band could
    have been drawn, and the margin is taken on the larger candidate set.
    -> step_ids, parent_ids, scores [T,B,W], lengths, log_probs [B,W] (the final state, float64), margin.
    The rank-gap margin is taken over the entries that are past their prefix at a step: inside it an entry has one finite
    candidate per carrying slot and its other slots follow the index rule of the all-(-inf) corner, so no rank is close."""
    from oracle import decoder_ref as dr
    from tests import beam_groups_ref as gref, beam_required_ref as rref, beam_sampling_ref as sref, beam_truncate_ref as tref
    from tests.test_gpu_ensemble import ref_select, ref_step_lp
    pfx = np.asarray(pfx, np.int32)
    B = fm.shape[0]
    assert pfx.shape[0] == B
    plen = prefix_lengths(pfx)
    cfg0 = members[0][1]
    V, end_id = cfg0.softmax_size, cfg0.end_id
    st = []
    for p, cfg in members:
        keys, values = dr.memory_projections(p, cfg, np.repeat(fm, W, axis=0))
        c, h, _ = dr.rnn_init(p, cfg, np.repeat(im, W, axis=0), None)
        st.append(dict(keys=keys, values=values, c=c, h=h, att=np.zeros((B * W, cfg.attn_size), np.float32)))
    if policy == 'beam':
        log_probs, finished, lengths = gref.init_state(B, W, 1)
    elif policy == 'groups':
        log_probs, finished, lengths = gref.init_state(B, W, G)
    elif policy == 'samples':
        log_probs, finished, lengths = sref.init_state(B, W)
        inv_temp = sref.inv_temp_of(temperature)
    else:
        assert policy == 'banks'
        req = np.asarray(req, np.int32)
        banks = req.shape[1] * S + 1
        log_probs, finished, lengths = rref.init_state(req, W, S)
    log_probs = log_probs.astype(np.float64)

    def select(lp, log_probs, finished, lengths, t, hists, keep):
        """The policy's step on the entries `keep` (a bool [B])."""
        a = (lp[keep], log_probs[keep], finished[keep], lengths[keep], end_id)
        if policy == 'beam':
            return ref_select(*a, 0.0)
        if policy == 'groups':
            return gref.ref_select_groups(*a, 0.0, G, lam)
        if policy == 'samples':
            return sref.ref_select_sampled(*a, sref.noise(seed, image_base, B, W, t, V)[2][keep], inv_temp)
        base, special = rref.table_of(hists, req, S, W)
        return rref.ref_select_banks(*a, 0.0, base[keep], special[keep], banks)

    ids = np.full(B * W, cfg0.start_id, np.int64)
    hists = [[] for _ in range(B * W)]
    out = dict(step_ids=[], parent_ids=[], scores=[])
    margin = np.inf
    everyone = np.ones(B, bool)
    truncated = policy == 'samples' and (top_k >= 1 or top_p < 1.0)
    agrees, band = True, 0
    for t in range(max_steps):
        logits = []
        for (p, cfg), s in zip(members, st):
            y, s['c'], s['h'], s['att'], _, _ = dr.decoder_step(p, cfg, s['keys'], s['values'], dr.embed(p['emb'], ids),
                                                                s['c'], s['h'], s['att'], None)
            logits.append((y @ p['W_o'] + p['b_o']).reshape(B, W, V))
        lp = ref_step_lp(np.stack(logits), wts)
        mask = np.zeros((B * W, V), bool)
        if cons:
            mask = ban_mask(hists, finished.reshape(-1), lengths.reshape(-1), V, end_id, **cons)
        mask = forced_mask(mask, pfx, finished, t, W).reshape(B, W, V)
        if truncated:
            tr = tref.truncate_ref(lp, finished, inv_temp, top_k, top_p, banned=mask)
            band = max(band, tr['band'])
            small = mask.copy()
            for (b, w), row in tr['rows'].items():
                if row is not None:
                    mask[b, w], small[b, w] = row['must_drop'], ~row['must_keep']
            with np.errstate(invalid='ignore'):
                narrow = select(np.where(small, -np.inf, lp), log_probs, finished, lengths, t, hists, everyone)
        lp = np.where(mask, -np.inf, lp)
        with np.errstate(invalid='ignore'):
            r = select(lp, log_probs, finished, lengths, t, hists, everyone)
            if truncated:
                agrees = agrees and np.array_equal(narrow['word'], r['word'])
            free = plen <= t
            if free.any():
                margin = min(margin, select(lp, log_probs, finished, lengths, t, hists, free)['margin'])
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
    res.update(lengths=lengths, log_probs=log_probs, margin=float(margin), hists=hists, sandwich_agrees=agrees, band=band)
    return res


def captions(res, b, slot):
    """The tokens of slot `slot` of image b after the tree gather of a result (predicted_ids [T,B,W], lengths)."""
    return res['predicted_ids'][:int(res['lengths'][b, slot]), b, slot].tolist()


def trace(ref, b, slot):
    """The same from a reference's step_ids / parent_ids, by walking the parents back."""
    T = ref['step_ids'].shape[0]
    seq, w = [], slot
    for t in range(T - 1, -1, -1):
        seq.append(int(ref['step_ids'][t, b, w]))
        w = int(ref['parent_ids'][t, b, w])
    return seq[::-1][:int(ref['lengths'][b, slot])]
