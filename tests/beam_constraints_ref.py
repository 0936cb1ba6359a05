"""Reference of constrained beam search for the tests: the ban rule as a plain function over a history list, and the
ensemble reference loop of tests/test_gpu_ensemble.py with that rule applied before the selection.

The rule (include/comic_hip.h, comic_beam_constraints): a live beam with history h[0..L-1] bans candidate v when v is
suppressed, when v is <EOS> and the beam is shorter than min_length, or when n > 0, L + 1 >= n, (L + 1) % s == 0 and a window
start i with i % s == 0 and i + n - 1 <= L - 1 has h[i..i+n-2] == h[L-n+1..L-1] and h[i+n-1] == v."""
import numpy as np


def ngram_bans(h, n, s=1):
    """Tokens whose emission after history `h` would repeat an n-gram whose window starts at a multiple of s."""
    h = [int(x) for x in h]
    L = len(h)
    out = set()
    if n <= 0 or L + 1 < n or (L + 1) % s != 0:
        return out
    tail = h[L - n + 1:L]                       # the n - 1 tokens the candidate would follow
    for i in range(0, L, s):
        if i + n - 1 > L - 1:
            break
        if h[i:i + n - 1] == tail:
            out.add(h[i + n - 1])
    return out


def banned(h, length, end_id, min_length=0, no_repeat_ngram=0, ngram_stride=1, suppress=()):
    """The banned set of a LIVE beam with history h and `length` emitted tokens (a finished beam bans nothing)."""
    out = set(int(v) for v in suppress)
    if length < min_length:
        out.add(int(end_id))
    return out | ngram_bans(h, no_repeat_ngram, ngram_stride)


def ban_mask(hists, finished, lengths, V, end_id, **cons):
    """bool [R, V] over rows with histories `hists`; finished rows are all False."""
    R = len(hists)
    m = np.zeros((R, V), bool)
    for r in range(R):
        if not finished[r]:
            m[r, sorted(banned(hists[r], int(lengths[r]), end_id, **cons))] = True
    return m


def pack_bits(mask):
    """bool [R, V] -> uint32 [R, ceil(V / 32)], bit v of word v // 32."""
    R, V = mask.shape
    words = (V + 31) // 32
    padded = np.zeros((R, words * 32), np.uint8)
    padded[:, :V] = mask
    return np.packbits(padded.reshape(R, words, 32), axis=2, bitorder='little').view('<u4').reshape(R, words)


def constrained_reference(members, wts, fm, im, W, max_steps, **cons):
    """ensemble_reference of tests/test_gpu_ensemble.py with lp[banned] = -inf for live beams before the selection and
    per-beam histories re-ordered by the chosen parents.  -> step_ids, parent_ids, scores [T,B,W], lengths, margin."""
    from oracle import decoder_ref as dr
    from tests.test_gpu_ensemble import ref_select, ref_step_lp
    B = fm.shape[0]
    cfg0 = members[0][1]
    V = cfg0.softmax_size
    st = []
    for p, cfg in members:
        keys, values = dr.memory_projections(p, cfg, np.repeat(fm, W, axis=0))
        c, h, _ = dr.rnn_init(p, cfg, np.repeat(im, W, axis=0), None)
        st.append(dict(keys=keys, values=values, c=c, h=h, att=np.zeros((B * W, cfg.attn_size), np.float32)))
    log_probs = np.full((B, W), -np.inf, np.float64)
    log_probs[:, 0] = 0
    finished = np.ones((B, W), np.int32)
    finished[:, 0] = 0
    lengths = np.zeros((B, W), np.int64)
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
        mask = ban_mask(hists, finished.reshape(-1), lengths.reshape(-1), V, cfg0.end_id, **cons).reshape(B, W, V)
        lp = np.where(mask, -np.inf, lp)
        r = ref_select(lp, log_probs, finished, lengths, cfg0.end_id, 0.0)
        margin = min(margin, r['margin'])
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
    res.update(lengths=lengths, margin=float(margin))
    return res
