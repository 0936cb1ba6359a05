"""Decoder.score (forward only, comic_decoder_score) against Decoder.train_step(training=False) -- what validation ran
before -- on ONE device in ONE process, at the decoder geometries of BASELINE configs[1] (COMIC-256: radix V = 258, 8 heads,
tied projection, batch 64) and configs[4] (word V = 25 599, 1 head, no feature-map projection, batch 50).  T' = 20.
Both sides replay their hipGraph (use_graph=True, as CaptionModel.run_eval_step calls them), the two are timed in
alternating rounds with device events, and the medians are reported: one JSON line.  ROUNDS (default 7), STEPS per round
(default 20), WARMUP (default 5)."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from comic_amd import decoder as cdec  # noqa: E402

ROUNDS, STEPS, WARMUP = (int(os.environ.get(k, d)) for k, d in (('ROUNDS', '7'), ('STEPS', '20'), ('WARMUP', '5')))
SHAPES = {
    'configs[1] COMIC-256 radix V=258 B=64': (cdec.DecoderSpec(), 64),
    'configs[4] word V=25599 B=50': (cdec.DecoderSpec(V=25599, token_type='word', H=1, fm_projection=None, start_id=25597,
                                                      end_id=25598), 50),
}
L_CAP = 21            # T = T' = 20


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(STEPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / STEPS


out = {}
for name, (spec, B) in SHAPES.items():
    rng = np.random.default_rng(0)
    fm = torch.from_numpy(rng.standard_normal((B, spec.M, spec.C)).astype(np.float32)).to('cuda:0')
    im = torch.from_numpy(rng.standard_normal((B, spec.Cg)).astype(np.float32)).to('cuda:0')
    caps = np.full((B, L_CAP), -1, np.int64)
    for b in range(B):
        n = L_CAP - 2 if b == 0 else 6 + b % 13
        caps[b, 0], caps[b, 1:1 + n], caps[b, 1 + n] = spec.start_id, rng.integers(0, min(spec.V - 2, 256), n), spec.end_id
    dec = cdec.Decoder(spec, None, 'cuda:0')
    step = lambda: dec.train_step(fm, im, caps, training=False, use_graph=True)      # noqa: E731
    score = lambda: dec.score(fm, im, caps, use_graph=True)                          # noqa: E731
    for _ in range(WARMUP):
        step()
        score()
    torch.cuda.synchronize()
    t_step, t_score = [], []
    for _ in range(ROUNDS):
        t_step.append(timed(step))
        t_score.append(timed(score))
    lib = dec.lib
    ms_step, ms_score = statistics.median(t_step), statistics.median(t_score)
    out[name] = {'train_step_eval_ms': round(ms_step, 4), 'score_ms': round(ms_score, 4),
                 'score_over_train_step': round(ms_score / ms_step, 4),
                 'train_step_ms_min_max': [round(min(t_step), 4), round(max(t_step), 4)],
                 'score_ms_min_max': [round(min(t_score), 4), round(max(t_score), 4)],
                 'score_path': int(lib.comic_decoder_score_path()), 'train_path': int(lib.comic_decoder_train_path()),
                 'score_workspace_bytes': int(dec._score_ctxs[(B, L_CAP - 1, L_CAP - 1, False)].nbytes),
                 'train_workspace_bytes': int(next(iter(dec._ctx.values())).nbytes)}
    del dec
    torch.cuda.empty_cache()
out['config'] = ('T = 20, hipGraph replay on both sides, median of %d alternating rounds of %d calls after %d warm-up calls, '
                 'device events' % (ROUNDS, STEPS, WARMUP))
print(json.dumps(out))
