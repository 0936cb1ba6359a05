"""What soft targets cost a decoder training step (Decoder.train_step(soft=, teacher=)) and what a teacher's table costs
(teacher_targets), on ONE device in ONE process under hipGraph replay of the step:
  hard .......... the step without soft targets (comic_decoder_train_step: the fused loss + map-loss launch)
  smooth ........ label smoothing 0.1 (comic_xent_soft + the two map-loss launches + the nll reduction)
  distil ........ label smoothing 0.1, teacher weight 0.5, K = 16 (the same launches, the table copied in front of the graph)
at the COMIC-256 radix geometry (B = 64, T = 20, V = 258) and at the word geometry (B = 50, T = 20, V = 25 599), and
  teacher1 / 3 .. teacher_targets of 1 / 3 members (their forward-only phases, eager launches, + one comic_teacher_topk)
The sides are timed in alternating rounds with device events around STEPS calls each and the medians are reported: one JSON
line, printed and written to OUT (default profiles/r21_soft_time.json).  ROUNDS (default 7), STEPS per round (default 20),
WARMUP rounds (default 2: the second call of a shape captures its graph)."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from comic_amd import decoder as cdec  # noqa: E402

ROUNDS, STEPS, WARMUP = (int(os.environ.get(k, d)) for k, d in (('ROUNDS', '7'), ('STEPS', '20'), ('WARMUP', '2')))
OUT = os.environ.get('OUT', os.path.join(ROOT, 'profiles', 'r21_soft_time.json'))
DEV = 'cuda:0'
GEOMETRIES = {
    'radix': (cdec.DecoderSpec(), 64),
    'word': (cdec.DecoderSpec(V=25599, token_type='word', H=1, fm_projection=None, start_id=25597, end_id=25598), 50)}
SMOOTH = cdec.SoftTargets(smoothing=0.1)
DISTIL = cdec.SoftTargets(smoothing=0.1, teacher_weight=0.5, top_k=16, temperature=2.0)


def batch(spec, B, L, seed):
    rng = np.random.default_rng(seed)
    fm = torch.from_numpy(rng.standard_normal((B, spec.M, spec.C)).astype(np.float32)).to(DEV)
    im = torch.from_numpy(rng.standard_normal((B, spec.Cg)).astype(np.float32)).to(DEV)
    caps = np.full((B, L), -1, np.int64)
    for b in range(B):
        n = L - 2 if b == 0 else int(rng.integers(5, L - 1))
        caps[b, 0] = spec.start_id
        caps[b, 1:1 + n] = rng.integers(0, min(spec.V - 2, 25000), n)
        caps[b, 1 + n] = spec.end_id
    return fm, im, caps


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(STEPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / STEPS * 1e3               # microseconds per call


out = {}
for name, (spec, B) in GEOMETRIES.items():
    fm, im, caps = batch(spec, B, 21, 3)                 # T = 20
    students = {k: cdec.Decoder(spec, None, DEV, seed=1) for k in ('hard', 'smooth', 'distil')}
    teachers = [cdec.Decoder(spec, None, DEV, seed=10 + k) for k in range(3)]
    ens = cdec.EnsembleDecoder(teachers)
    table = tuple(t.clone() for t in teachers[0].teacher_targets(fm, im, caps, DISTIL.top_k, DISTIL.temperature))
    sides = dict(
        hard=lambda: students['hard'].train_step(fm, im, caps, training=True, use_graph=True),
        smooth=lambda: students['smooth'].train_step(fm, im, caps, training=True, use_graph=True, soft=SMOOTH),
        distil=lambda: students['distil'].train_step(fm, im, caps, training=True, use_graph=True, soft=DISTIL, teacher=table),
        teacher1=lambda: teachers[0].teacher_targets(fm, im, caps, DISTIL.top_k, DISTIL.temperature),
        teacher3=lambda: ens.teacher_targets(fm, im, caps, DISTIL.top_k, DISTIL.temperature))
    for _ in range(WARMUP):
        for fn in sides.values():
            timed(fn)
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, fn in sides.items():
            times[k].append(timed(fn))
    for k, d in students.items():
        assert bool(torch.isfinite(d.grads.flat).all()), (name, k)
    med = {k: statistics.median(x) for k, x in times.items()}
    geo = {k + '_us': round(x, 1) for k, x in med.items()}
    geo.update({k + '_us_min_max': [round(min(x), 1), round(max(x), 1)] for k, x in times.items()})
    geo.update(smooth_minus_hard_us=round(med['smooth'] - med['hard'], 1), distil_minus_hard_us=round(med['distil'] - med['hard'], 1),
               B=B, T=20, V=spec.V, train_path=students['hard'].lib.comic_decoder_train_path())
    out[name] = geo
out['config'] = ('decoder training steps replayed from their hipGraphs (dropout on, device-generated masks), teacher_targets as '
                 'eager launches; median of %d alternating rounds of %d calls after %d warm-up rounds, device events, one '
                 'process' % (ROUNDS, STEPS, WARMUP))
line = json.dumps(out)
print(line)
with open(OUT, 'w') as f:
    f.write(line + '\n')
