"""Reference of sampling inside the beam step for the tests, in numpy: the generator (splitmix64 in uint64, the 23-bit
draw, the Gumbel noise in float64), one sampled step (ref_select_sampled), and the ensemble reference loop of
tests/beam_groups_ref.diverse_reference with the sampled selection (sampled_reference).

The rule (include/comic_hip.h, comic_beam_sampling): the W slots of an entry are W independent chains, all live from the
start.  For entry b, slot w, step t, candidate v:
    k1 = splitmix64(splitmix64(seed) ^ (image_base + b));  k2 = splitmix64(k1 ^ ((w << 32) | t))
    r = splitmix64(k2 ^ v);  k = r >> 41;  u = (2k + 1) * 2^-24;  g = -log(-log(u))
A live slot ranks rank[v] = lp[v] * inv_temp + g with inv_temp the fp32 value of 1 / temperature and takes its best
candidate (lowest v on ties); a finished slot sees no noise and emits <EOS>.  word = v, parent = w, scores = the state =
old state + lp[v]: the unperturbed, untempered log-probability.

Margin rule: that of tests/test_gpu_ensemble.py, per slot -- in every entry and every LIVE slot the float64 best and
second-best rank differ by more than GAP * max(1, |rank|); margin is the smallest such ratio, > 1 claims every id."""
import functools

import numpy as np

from tests import regimes
from tests.test_gpu_ensemble import F32_MIN, GAP, ref_step_lp, step_case

_C0, _C1, _C2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def splitmix64(z):
    """csrc/splitmix.h on a uint64 array (wrapping arithmetic)."""
    z = np.atleast_1d(np.asarray(z, np.uint64))
    with np.errstate(over='ignore'):
        z = z + _C0
        z = (z ^ (z >> np.uint64(30))) * _C1
        z = (z ^ (z >> np.uint64(27))) * _C2
    return z ^ (z >> np.uint64(31))


def noise(seed, image_base, B, W, t, V):
    """-> k [B,W,V] int64 (< 2^23), u [B,W,V] float64 (the exact value of the fp32 u), g [B,W,V] float64."""
    with np.errstate(over='ignore'):
        k1 = splitmix64(splitmix64(np.uint64(seed)) ^ (np.uint64(image_base) + np.arange(B, dtype=np.uint64)))       # [B]
        wt = (np.arange(W, dtype=np.uint64) << np.uint64(32)) | np.uint64(t)
        k2 = splitmix64((k1[:, None] ^ wt[None, :]).reshape(-1)).reshape(B, W)
        r = splitmix64((k2[:, :, None] ^ np.arange(V, dtype=np.uint64)[None, None, :]).reshape(-1)).reshape(B, W, V)
    k = (r >> np.uint64(41)).astype(np.int64)
    u = (2 * k + 1).astype(np.float64) * 2.0 ** -24
    return k, u, -np.log(-np.log(u))


def inv_temp_of(temperature):
    """1.0f / temperature as the host forms it, in fp32."""
    return np.float32(1.0) / np.float32(temperature)


def ref_select_sampled(lp, log_probs, finished, lengths, end_id, g, inv_temp):
    """One sampled step on the step distribution lp [B,W,V] (float64; -inf where a live slot is banned) with the noise g
    [B,W,V].  -> dict(word, parent, scores, log_probs, finished, lengths, margin, greedy) as tests/test_gpu_ensemble
    .ref_select; greedy [B,W] is the choice of a step that ignored the noise."""
    B, W, V = lp.shape
    lengths = np.asarray(lengths, np.int64)
    fin = np.asarray(finished, bool)
    fin_row = np.full(V, F32_MIN, np.float64)
    fin_row[end_id] = 0
    step = np.where(fin[:, :, None], fin_row[None, None, :], lp)
    total = np.asarray(log_probs, np.float64)[:, :, None] + step
    with np.errstate(invalid='ignore'):
        rank = np.where(fin[:, :, None], total, lp * np.float64(inv_temp) + g)
    order = np.argsort(-rank, axis=2, kind='stable')[:, :, :2]
    top = np.take_along_axis(rank, order, axis=2)
    with np.errstate(invalid='ignore'):
        ratio = (top[:, :, 0] - top[:, :, 1]) / (GAP * np.maximum(1.0, np.abs(top[:, :, 0])))
    live = ~fin
    margin = float(ratio[live].min()) if live.any() else np.inf
    word = order[:, :, 0].astype(np.int32)
    parent = np.tile(np.arange(W, dtype=np.int32), (B, 1))
    new_lp = np.take_along_axis(total, word[:, :, None].astype(np.int64), axis=2)[:, :, 0]
    return dict(word=word, parent=parent, scores=new_lp, log_probs=new_lp,
                finished=(fin | (word == end_id)).astype(np.int32), lengths=lengths + live.astype(np.int64), margin=margin,
                greedy=np.argmax(np.where(fin[:, :, None], total, lp), axis=2).astype(np.int32))


def init_state(B, W):
    """Every slot live with log-probability 0."""
    return np.zeros((B, W), np.float32), np.zeros((B, W), np.int32), np.zeros((B, W), np.int64)


@functools.lru_cache(maxsize=None)
def sampled_inputs(shape, state):
    """The inputs of tests/test_gpu_ensemble.step_case (logits 2 N(0,1) from default_rng(0), the Dirichlet weights, the `mid`
    state with one finished slot per entry as drawn there), with every slot live at log-probability 0 for `init`; lp is the
    float64 step distribution."""
    c = step_case(shape, state, 0.0)
    c = {k: c[k] for k in ('logits', 'wts', 'end_id', 'log_probs', 'finished', 'lengths')}
    if state == 'init':
        c['log_probs'], c['finished'], c['lengths'] = init_state(shape[1], shape[2])
    c['lp'] = ref_step_lp(c['logits'], c['wts'])
    return c


def peaked_inputs(shape, state='mid'):
    """sampled_inputs with the members' logits in the regime `peaked` of tests/regimes.py (rows 30 N(0,1) + 200 / - 200
    with a dominant entry, another one in every member), lp the float64 step distribution of these; a fresh dict whose
    logits the caller may edit (recompute lp then)"""
    n, B, W, V = shape
    c = dict(sampled_inputs(shape, state))
    c['logits'] = regimes.peaked_logits(np.random.default_rng(V), n * B * W, V)[0].reshape(n, B, W, V)
    c['lp'] = ref_step_lp(c['logits'], c['wts'])
    return c


@functools.lru_cache(maxsize=None)
def sampled_case(shape, state, temperature, seed=5, image_base=0, t=0):
    """sampled_inputs + the float64 reference (`ref`), computed once and shared."""
    c = dict(sampled_inputs(shape, state))
    n, B, W, V = shape
    g = noise(seed, image_base, B, W, t, V)[2]
    c['ref'] = ref_select_sampled(c['lp'], c['log_probs'], c['finished'], c['lengths'], c['end_id'], g,
                                  inv_temp_of(temperature))
    return c


def sampled_reference(members, wts, fm, im, W, max_steps, seed, temperature, image_base=0, **cons):
    """diverse_reference of tests/beam_groups_ref.py with every slot live at the start and the sampled selection (cons
    empty: no bans).  -> step_ids, parent_ids, scores [T,B,W], lengths, log_probs [B,W] (the final state), margin."""
    from oracle import decoder_ref as dr
    from tests.beam_constraints_ref import ban_mask
    B = fm.shape[0]
    cfg0 = members[0][1]
    V = cfg0.softmax_size
    inv_temp = inv_temp_of(temperature)
    st = []
    for p, cfg in members:
        keys, values = dr.memory_projections(p, cfg, np.repeat(fm, W, axis=0))
        c, h, _ = dr.rnn_init(p, cfg, np.repeat(im, W, axis=0), None)
        st.append(dict(keys=keys, values=values, c=c, h=h, att=np.zeros((B * W, cfg.attn_size), np.float32)))
    log_probs, finished, lengths = init_state(B, W)
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
        r = ref_select_sampled(lp, log_probs, finished, lengths, cfg0.end_id, noise(seed, image_base, B, W, t, V)[2], inv_temp)
        margin = min(margin, r['margin'])
        if cons:
            assert not mask[np.arange(B)[:, None], r['parent'], r['word']].any(), 'the reference selected a banned token'
        log_probs, finished, lengths = r['log_probs'], r['finished'], r['lengths']
        hists = [h + [int(w)] for h, w in zip(hists, r['word'].reshape(-1))]      # (a slot's parent is the slot itself)
        out['step_ids'].append(r['word']); out['parent_ids'].append(r['parent']); out['scores'].append(r['scores'])
        ids = r['word'].reshape(-1).astype(np.int64)
        if finished.all():
            break
    res = {k: np.stack(v) for k, v in out.items()}
    res.update(lengths=lengths, log_probs=log_probs, margin=float(margin))
    return res
