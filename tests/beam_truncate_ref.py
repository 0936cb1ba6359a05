"""Reference of the top-k / nucleus truncation of the sampled step for the tests, in numpy float64 (the rule:
include/comic_hip.h, comic_beam_truncation), on lp from tests.test_gpu_ensemble.ref_step_lp and the inputs of
tests.beam_sampling_ref.sampled_inputs.

For a live row with a[v] = lp[v] * inv_temp (inv_temp the fp32 value of 1 / temperature) and the allowed set A (ban bit
clear):  top-k keeps the top_k largest a over A, lowest v on ties (top_k >= |A|: all of A);  top-p keeps, of those, every
token with a >= tau, tau the largest value whose tie-inclusive mass from the top reaches top_p * Z;  everything else gets its
ban bit set.  A row without a finite maximum over A, and a finished row, are left as they came.

An fp32 kernel cannot be asked to agree with float64 on a token whose cumulative mass sits within rounding of top_p, so the
reference returns, per live row, a SANDWICH:
    must_keep ... kept under both top_p * (1 - GAP) and top_p * (1 + GAP), and above the k-th value a_k by more than
                  GAP * max(1, |a_k|)
    must_drop ... dropped under both, or below a_k by more than that, or banned
    band ........ the rest
GAP = 1e-4 is the project's constant (tests/test_gpu_ensemble.py); a numpy fp32 emulation at V = 9001 puts the fp32 error of
cum / Z at 3.7e-6.  Values tied in float64 move as one group.  Where a_k and the (k+1)-th value are more than the gap apart
(`k_clear`), no fp32 rounding can swap them: the k stage then has no band at all, K is the exact set, and only the p stage
has one -- the combined k-then-p cases need that, because their nucleus is taken on K.

A device mask passes (check_mask) iff in EVERY live row it keeps all of must_keep, keeps none of must_drop, with top-k alone
keeps exactly min(top_k, |A|) tokens, and leaves finished rows and pre-set bits as they were.  No row is excused; the band
holds at most BAND_CAP tokens in every row and must_keep is never empty, asserted there, so a loose band cannot hide a
failure."""
import numpy as np

from tests.test_gpu_ensemble import GAP

BAND_CAP = 8


def _nucleus(a_sorted, p):
    """The number of leading tokens of a_sorted (descending) the nucleus at p keeps: through the end of the first tie group
    whose inclusive mass reaches p * Z."""
    if p >= 1.0:
        return a_sorted.size
    e = np.exp(a_sorted - a_sorted[0])
    cum = np.cumsum(e)
    ends = np.flatnonzero(np.r_[a_sorted[1:] != a_sorted[:-1], True])
    hit = cum[ends] >= p * cum[-1]
    return int(ends[np.argmax(hit)] if hit.any() else ends[-1]) + 1


def truncate_row(a, allowed, top_k, top_p):
    """a float64 [V], allowed bool [V] -> None when the row is left as it came, else dict(exact, must_keep, must_drop bool
    [V], k_clear, n_allowed)."""
    idx = np.flatnonzero(allowed)
    if idx.size == 0 or not np.isfinite(a[idx].max()) or np.isnan(a[idx]).any():
        return None
    order = idx[np.lexsort((idx, -a[idx]))]                     # value descending, v ascending
    V = a.size
    k_on = 1 <= top_k < idx.size
    keep_k, drop_k, k_clear = allowed.copy(), ~allowed, True
    K = order
    if k_on:
        K = order[:top_k]
        a_k, a_next = a[order[top_k - 1]], a[order[top_k]]
        gap = GAP * max(1.0, abs(a_k))
        k_clear = bool(a_k - a_next > gap)
        if k_clear:
            keep_k = np.zeros(V, bool)
            keep_k[K] = True
            drop_k = ~keep_k
        else:
            keep_k = allowed & (a > a_k + gap)
            drop_k = ~allowed | (a < a_k - gap)
    exact = np.zeros(V, bool)
    keep_lo, keep_hi = np.ones(V, bool), np.ones(V, bool)
    if top_p < 1.0:
        aK = a[K]
        exact[K[:_nucleus(aK, top_p)]] = True
        keep_lo[:] = False
        keep_lo[K[:_nucleus(aK, top_p * (1 - GAP))]] = True
        keep_hi[:] = False
        keep_hi[K[:_nucleus(aK, top_p * (1 + GAP))]] = True
    else:
        exact[K] = True
    return dict(exact=exact, must_keep=keep_lo & keep_k, must_drop=~keep_hi | drop_k, k_clear=k_clear, n_allowed=int(idx.size))


def truncate_ref(lp, finished, inv_temp, top_k, top_p, banned=None):
    """lp float64 [B,W,V], finished [B,W], banned bool [B,W,V] or None -> dict(rows: per (b, w) None (finished, or left as it
    came) or truncate_row's dict; live bool [B,W]; band: the largest band over the rows; k_clear: over all rows)."""
    B, W, V = lp.shape
    a = np.asarray(lp, np.float64) * np.float64(np.float32(inv_temp))
    rows, band, k_clear, keep_min = {}, 0, True, V
    for b in range(B):
        for w in range(W):
            allowed = np.ones(V, bool) if banned is None else ~banned[b, w]
            r = None if finished[b, w] else truncate_row(a[b, w], allowed, top_k, top_p)
            rows[b, w] = r
            if r is not None:
                band = max(band, int((~r['must_keep'] & ~r['must_drop']).sum()))
                keep_min = min(keep_min, int(r['must_keep'].sum()))
                k_clear = k_clear and r['k_clear']
    return dict(rows=rows, band=band, k_clear=k_clear, keep_min=keep_min, live=np.asarray(finished) == 0)


def unpack_bits(bits, V):
    """uint32 [R, words] -> bool [R, V] (bit v of word v // 32); asserts that the bits at positions >= V are zero."""
    bits = np.ascontiguousarray(bits, '<u4')
    full = np.unpackbits(bits.view(np.uint8), axis=1, bitorder='little').astype(bool)
    assert not full[:, V:].any(), 'a bit at a position >= V is set'
    return full[:, :V]


def check_mask(dropped, ref, top_k, top_p, banned=None, exact=False):
    """dropped bool [B,W,V]: the device mask read back.  The pass rule of the module docstring; exact=True also asks for the
    float64 rule's own set, bit for bit (the tie cases, whose keys are equal to the bit on both sides)."""
    B, W, V = dropped.shape
    assert ref['band'] <= BAND_CAP, 'the band of this case holds %d tokens: it could hide a failure' % ref['band']
    assert ref['keep_min'] >= 1
    for (b, w), r in ref['rows'].items():
        was = np.zeros(V, bool) if banned is None else banned[b, w]
        got = dropped[b, w]
        if r is None:                                           # finished, or left as it came
            np.testing.assert_array_equal(got, was, err_msg='row (%d, %d) should be left as it came' % (b, w))
            continue
        assert got[was].all(), 'row (%d, %d): a bit that was set is clear' % (b, w)
        assert not got[r['must_keep']].any(), 'row (%d, %d) drops %s of must_keep' % (b, w, np.flatnonzero(got & r['must_keep']))
        assert got[r['must_drop']].all(), 'row (%d, %d) keeps %s of must_drop' % (b, w, np.flatnonzero(~got & r['must_drop']))
        if top_k >= 1 and top_p >= 1.0:
            assert int((~got).sum()) == min(top_k, r['n_allowed']), 'row (%d, %d) keeps %d tokens' % (b, w, (~got).sum())
        if exact:
            np.testing.assert_array_equal(~got, r['exact'], err_msg='row (%d, %d)' % (b, w))
