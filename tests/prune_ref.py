"""numpy reference of the mask event of `--prune_sparsity` (comic_prune_select): per group, `np.lexsort` on (flat index,
key) with the already pruned elements first; the first k of that order are pruned afterwards.  Shared by test_prune_cpu.py
(against a brute-force loop) and test_gpu_prune.py (against the device, bit for bit)."""
import numpy as np

ALIGN = 64          # decoder.FlatParams.ALIGN: every segment starts on a multiple of it


def keys(w):
    """The IEEE bits of |w|: -0.0 and +0.0 tie, +x and -x tie, denormals order below every normal number."""
    return np.ascontiguousarray(w, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def group_indices(segments, g):
    """Flat indices of group g's elements, ascending; segments: [(first, count, group)]."""
    return np.concatenate([np.arange(f, f + n, dtype=np.int64) for f, n, gg in segments if gg == g] or
                          [np.zeros(0, np.int64)])


def select(w, live, segments, targets):
    """-> the live flags after the event (a copy).  live: bool per flat element; targets[g]: pruned elements of group g
    afterwards.  A target that is not above the pruned count changes nothing."""
    out = np.array(live, bool, copy=True)
    key = keys(w)
    for g, k in enumerate(targets):
        idx = group_indices(segments, g)
        order = np.lexsort((idx, key[idx], out[idx]))        # last key first: pruned (False), then |w| bits, then index
        out[idx[order[:max(0, min(int(k), idx.size))]]] = False
    return out


def select_brute(w, live, segments, targets):
    """The same by definition: while fewer than k are pruned, prune the live element of smallest (key, index)."""
    out = np.array(live, bool, copy=True)
    key = keys(w)
    for g, k in enumerate(targets):
        idx = group_indices(segments, g)
        while int((~out[idx]).sum()) < min(int(k), idx.size):
            best = None
            for i in idx:
                if out[i] and (best is None or (int(key[i]), int(i)) < (int(key[best]), int(best))):
                    best = i
            out[best] = False
    return out


def pack(live):
    """bool per element -> uint32 words, bit i % 32 of word i / 32."""
    live = np.asarray(live, bool)
    pad = (-live.size) % 32
    return np.packbits(np.concatenate([live, np.ones(pad, bool)]), bitorder='little').view('<u4').copy()


def unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words, '<u4').view(np.uint8), bitorder='little')[:n].astype(bool)


def layout(sizes):
    """Offsets of segments padded to ALIGN floats, and the total -- FlatParams' rule."""
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off += (n + ALIGN - 1) // ALIGN * ALIGN
    return offs, off


def apply(bufs, live_before, live_after):
    """What the event does to w, m, v, shadow: +0.0f exactly at the newly pruned elements."""
    new = np.asarray(live_before, bool) & ~np.asarray(live_after, bool)
    out = []
    for b in bufs:
        b = np.array(b, np.float32, copy=True)
        b[new] = np.float32(0.0)
        out.append(b)
    return out
