"""What `--prune_sparsity` costs, on ONE device in ONE process, at the COMIC-256 decoder's parameter count (the flat buffer of
DecoderSpec(), about 22.8 MB), at a half-pruned mask:
  gated / masked ......... comic_adam_tf_gated against comic_adam_tf_masked without a shadow (7 floats moved per live parameter;
                           the mask adds 1/32 of a word)
  ema / masked_ema ....... comic_adam_tf_ema against comic_adam_tf_masked with the shadow (9 floats)
  event_layer / _global .. one mask event (comic_prune_select: 4 histogram passes, the tie count and the apply pass over the
                           prunable variables) per variable and over all of them together; the mask is reset to all-live and
                           the variables are restored in front of every timed event (outside the timed region), the target is
                           half of every group
The four launches are timed in alternating rounds with device events around LAUNCHES launches each, the events one at a time
in the same rounds; medians are reported: one JSON line, printed and written to OUT (default profiles/r22_prune_time.json).
ROUNDS (default 9), LAUNCHES per round (default 50), WARMUP rounds (default 2)."""
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from comic_amd import _lib as L, decoder as cdec, prune  # noqa: E402

ROUNDS, LAUNCHES, WARMUP = (int(os.environ.get(k, d)) for k, d in (('ROUNDS', '9'), ('LAUNCHES', '50'), ('WARMUP', '2')))
OUT = os.environ.get('OUT', os.path.join(ROOT, 'profiles', 'r22_prune_time.json'))
DEV = 'cuda:0'

lib = L.load()
P = cdec.FlatParams(cdec.DecoderSpec().param_shapes(), DEV, status_tail=True)
G, M, V, S = P.like(), P.like(), P.like(), P.like()
gen = torch.Generator(device='cpu').manual_seed(0)
P.flat.copy_(torch.randn(P.numel, generator=gen))
G.flat.copy_(1e-3 * torch.randn(P.numel, generator=gen))
S.flat.copy_(P.flat)
W0 = P.flat.clone()
n, t, omd = P.numel, 1000, 1e-3
lr_t = 1e-3 * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
w, g, m, v, s = (x.data.data_ptr() for x in (P, G, M, V, S))
flag = G.status.data_ptr()
masks = {scope: prune.PruneMask(P, prune.PruneSpec(0.5, 0, 1, 1, scope)) for scope in prune.SCOPES}
half = prune.PruneMask(P, prune.PruneSpec(0.5, 0, 1, 1, 'layer'))           # the mask of the timed launches: half pruned
half.select(half.targets_at(0.5), M, V, S)
P.flat.copy_(W0)
S.flat.copy_(W0)
half.mask_buffer(P)
half.mask_buffer(S)
words = half.words.data_ptr()
torch.cuda.synchronize()
pruned = sum(half.pruned_counts().values())


def gated():
    L.check(lib.comic_adam_tf_gated(w, g, m, v, n, lr_t, 0.9, 0.999, 1e-2, 1e-5, 1.0, flag, L.stream_ptr()), 'gated')


def masked():
    L.check(lib.comic_adam_tf_masked(w, g, m, v, n, lr_t, 0.9, 0.999, 1e-2, 1e-5, 1.0, flag, None, 0.0, words, 0,
                                     L.stream_ptr()), 'masked')


def ema():
    L.check(lib.comic_adam_tf_ema(w, g, m, v, n, lr_t, 0.9, 0.999, 1e-2, 1e-5, 1.0, flag, s, omd, L.stream_ptr()), 'ema')


def masked_ema():
    L.check(lib.comic_adam_tf_masked(w, g, m, v, n, lr_t, 0.9, 0.999, 1e-2, 1e-5, 1.0, flag, s, omd, words, 0,
                                     L.stream_ptr()), 'masked_ema')


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / LAUNCHES * 1e3            # microseconds per call


def timed_event(scope):
    mk = masks[scope]
    mk.words.fill_(-1)
    P.flat.copy_(W0)
    mk.targets.copy_(torch.tensor(mk.targets_at(0.5), dtype=torch.int64))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    L.check(lib.comic_prune_select(w, mk.words.data_ptr(), mk.n_total, mk.table.data_ptr(), len(mk.segments),
                                   mk.targets.data_ptr(), mk.n_groups, m, v, s, mk.workspace.data_ptr(), mk.workspace.numel(),
                                   L.stream_ptr()), 'event')
    b.record()
    b.synchronize()
    assert sum(mk.pruned_counts().values()) == sum(mk.targets_at(0.5))
    return a.elapsed_time(b) * 1e3


sides = dict(gated=gated, masked=masked, ema=ema, masked_ema=masked_ema)
for _ in range(WARMUP):
    for fn in sides.values():
        timed(fn)
    for scope in masks:
        timed_event(scope)
# the events rewrote the variables: back to the half-pruned state of the launches
P.flat.copy_(W0)
half.mask_buffer(P)
torch.cuda.synchronize()
times = {k: [] for k in list(sides) + ['event_' + sc for sc in masks]}
for _ in range(ROUNDS):
    for k, fn in sides.items():
        times[k].append(timed(fn))
for _ in range(ROUNDS):
    for scope in masks:
        times['event_' + scope].append(timed_event(scope))
assert bool(torch.isfinite(P.flat).all()) and bool(torch.isfinite(S.flat).all())
med = {k: statistics.median(x) for k, x in times.items()}
out = {k + '_us': round(x, 2) for k, x in med.items()}
out.update({k + '_us_min_max': [round(min(x), 2), round(max(x), 2)] for k, x in times.items()})
out.update(
    masked_over_gated=round(med['masked'] / med['gated'], 4), masked_ema_over_ema=round(med['masked_ema'] / med['ema'], 4),
    event_layer_passes_of_23mb=round(med['event_layer'] / (4 * n / 1e6 / 4.0), 2),
    elements=n, megabytes=round(4 * n / 1e6, 2), prunable_elements=sum(half.group_sizes), pruned_in_timed_mask=pruned,
    groups_layer=masks['layer'].n_groups,
    config=('COMIC-256 decoder flat buffer, Adam, status word present and clear, half of every prunable variable pruned; the '
            'launches back to back on one stream, median of %d alternating rounds of %d launches after %d warm-up rounds; the '
            'events one at a time from an all-live mask towards 0.5, median of %d; device events; '
            'event_layer_passes_of_23mb: the event in units of one read of the buffer at 4 TB/s' % (ROUNDS, LAUNCHES, WARMUP,
                                                                                                     ROUNDS)))
line = json.dumps(out)
print(line)
with open(OUT, 'w') as f:
    f.write(line + '\n')
