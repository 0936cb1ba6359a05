"""The moving-average shadow of `--ema_decay` inside the Adam launch (comic_adam_tf_ema) against the launch without it, on
ONE device in ONE process, at the COMIC-256 decoder's parameter count (the flat buffer of DecoderSpec(), about 22.8 MB):
  gated ......... comic_adam_tf_gated, what a run without --ema_decay launches (7 floats moved per parameter)
  ema ........... comic_adam_tf_ema, the shadow updated in the same launch (9 floats per parameter)
  gated_then_pass the gated launch followed by a separate pass over shadow and variables (torch's in-place lerp: 3 more
                  floats per parameter and a second launch) -- for context: what keeping the average outside costs
All three run with the status word of a gradient buffer (not set), are timed in alternating rounds with device events around
LAUNCHES launches each, and the medians are reported: one JSON line, printed and written to OUT (default
profiles/r16_ema_time.json).  ROUNDS (default 9), LAUNCHES per round (default 50: 450 timed launches a form), WARMUP rounds
(default 2).  STEP_MS: the decoder step the share is quoted against (default 1.15, README)."""
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from comic_amd import _lib as L, decoder as cdec  # noqa: E402

ROUNDS, LAUNCHES, WARMUP = (int(os.environ.get(k, d)) for k, d in (('ROUNDS', '9'), ('LAUNCHES', '50'), ('WARMUP', '2')))
STEP_MS = float(os.environ.get('STEP_MS', '1.15'))
OUT = os.environ.get('OUT', os.path.join(ROOT, 'profiles', 'r16_ema_time.json'))
DEV = 'cuda:0'

lib = L.load()
P = cdec.FlatParams(cdec.DecoderSpec().param_shapes(), DEV, status_tail=True)
G, M, V, S = P.like(), P.like(), P.like(), P.like()
gen = torch.Generator(device='cpu').manual_seed(0)
P.flat.copy_(torch.randn(P.numel, generator=gen))
G.flat.copy_(1e-3 * torch.randn(P.numel, generator=gen))
S.flat.copy_(P.flat)
n, t, omd = P.numel, 1000, 1e-3
lr_t = 1e-3 * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
w, g, m, v, s = (x.data.data_ptr() for x in (P, G, M, V, S))
flag = G.status.data_ptr()


def gated():
    L.check(lib.comic_adam_tf_gated(w, g, m, v, n, lr_t, 0.9, 0.999, 1e-2, 1e-5, 1.0, flag, L.stream_ptr()), 'gated')


def ema():
    L.check(lib.comic_adam_tf_ema(w, g, m, v, n, lr_t, 0.9, 0.999, 1e-2, 1e-5, 1.0, flag, s, omd, L.stream_ptr()), 'ema')


def gated_then_pass():
    gated()
    S.flat.lerp_(P.flat, omd)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / LAUNCHES * 1e3            # microseconds per call


sides = dict(gated=gated, ema=ema, gated_then_pass=gated_then_pass)
for _ in range(WARMUP):
    for fn in sides.values():
        timed(fn)
torch.cuda.synchronize()
times = {k: [] for k in sides}
for _ in range(ROUNDS):
    for k, fn in sides.items():
        times[k].append(timed(fn))
assert bool(torch.isfinite(P.flat).all()) and bool(torch.isfinite(S.flat).all())
med = {k: statistics.median(x) for k, x in times.items()}
out = {k + '_us': round(x, 2) for k, x in med.items()}
out.update({k + '_us_min_max': [round(min(x), 2), round(max(x), 2)] for k, x in times.items()})
out.update(
    ema_minus_gated_us=round(med['ema'] - med['gated'], 2), ema_over_gated=round(med['ema'] / med['gated'], 4),
    pass_minus_gated_us=round(med['gated_then_pass'] - med['gated'], 2),
    ema_share_of_step=round((med['ema'] - med['gated']) / (STEP_MS * 1e3), 4),
    gated_gb_per_s=round(7 * 4 * n / med['gated'] / 1e3, 1), ema_gb_per_s=round(9 * 4 * n / med['ema'] / 1e3, 1),
    elements=n, megabytes=round(4 * n / 1e6, 2),
    config=('COMIC-256 decoder flat buffer, Adam, status word present and clear, back-to-back launches on one stream, median '
            'of %d alternating rounds of %d launches after %d warm-up rounds, device events; share against a %.2f ms decoder '
            'step' % (ROUNDS, LAUNCHES, WARMUP, STEP_MS)))
line = json.dumps(out)
print(line)
with open(OUT, 'w') as f:
    f.write(line + '\n')
