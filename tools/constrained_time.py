"""Constrained beam search (Decoder.beam_search(constraints=), comic_decoder_beam_constrained) against the two unconstrained
decodes it can be compared with, on ONE device in ONE process: beam 3 at the word geometry of BASELINE configs[4]
(V = 25 599, 1 head, no feature-map projection, batch 50), MAX_STEPS decode steps (default 20; random weights never emit
EOS, so every step executes), constraints min_length = 8, no_repeat_ngram = 3.
  (a) constrained ....... Decoder.beam_search(constraints=): the ensemble executor with one member, plus the ban kernel and
                          the ban policy of the step
  (b) ensemble of one ... EnsembleDecoder([dec]).beam_search, unconstrained: the same executor without either
  (c) streaming ......... Decoder.beam_search, unconstrained: the single-model path whose logits are never written
All three replay their hipGraph and return the same dict (want_attention=False), are timed in alternating rounds with
device events, and the medians are reported: one JSON line, printed and written to OUT (default
profiles/r10_constrained_time.json).  ROUNDS (default 7), STEPS calls per round (default 5), WARMUP (default 3)."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from comic_amd import decoder as cdec  # noqa: E402

ROUNDS, STEPS, WARMUP, MAX_STEPS = (int(os.environ.get(k, d)) for k, d in (('ROUNDS', '7'), ('STEPS', '5'), ('WARMUP', '3'),
                                                                          ('MAX_STEPS', '20')))
OUT = os.environ.get('OUT', os.path.join(ROOT, 'profiles', 'r10_constrained_time.json'))
B, W = 50, 3
spec = cdec.DecoderSpec(V=25599, token_type='word', H=1, fm_projection=None, start_id=25597, end_id=25598)
cons = cdec.BeamConstraints(min_length=8, no_repeat_ngram=3)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(STEPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / STEPS


rng = np.random.default_rng(0)
fm = torch.from_numpy(rng.standard_normal((B, spec.M, spec.C)).astype(np.float32)).to('cuda:0')
im = torch.from_numpy(rng.standard_normal((B, spec.Cg)).astype(np.float32)).to('cuda:0')
dec = cdec.Decoder(spec, None, 'cuda:0', seed=0)
ens = cdec.EnsembleDecoder([dec])
steps = []
sides = {
    'constrained': lambda: steps.append(
        dec.beam_search(fm, im, W, MAX_STEPS, want_attention=False, constraints=cons)['step_ids'].shape[0]),
    'ensemble_of_one': lambda: steps.append(ens.beam_search(fm, im, W, MAX_STEPS)['step_ids'].shape[0]),
    'streaming': lambda: steps.append(dec.beam_search(fm, im, W, MAX_STEPS, want_attention=False)['step_ids'].shape[0]),
}
for _ in range(WARMUP):
    for fn in sides.values():
        fn()
torch.cuda.synchronize()
times = {k: [] for k in sides}
for _ in range(ROUNDS):
    for k, fn in sides.items():
        times[k].append(timed(fn))
assert set(steps) == {MAX_STEPS}, 'a decode ended early: the sides did not run the same number of steps'
med = {k: statistics.median(v) for k, v in times.items()}
out = {k + '_ms': round(v, 4) for k, v in med.items()}
out.update({k + '_ms_min_max': [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})
out.update(
    constrained_over_ensemble_of_one=round(med['constrained'] / med['ensemble_of_one'], 4),
    constrained_over_streaming=round(med['constrained'] / med['streaming'], 4),
    constrained_ms_per_step=round(med['constrained'] / MAX_STEPS, 4),
    ensemble_of_one_ms_per_step=round(med['ensemble_of_one'] / MAX_STEPS, 4),
    streaming_ms_per_step=round(med['streaming'] / MAX_STEPS, 4),
    single_beam_path=int(dec.lib.comic_decoder_beam_path()),
    constrained_workspace_bytes=int(next(iter(dec._self_ensemble._ctxs.values())).nbytes),
    ensemble_workspace_bytes=int(next(iter(ens._ctxs.values())).nbytes),
    config=('word geometry V = 25599, B = 50, beam 3, %d steps, constraints min_length = 8, no_repeat_ngram = 3, hipGraph replay on '
            'all sides, host post-processing of beam_search included, median of %d alternating rounds of %d calls after %d '
            'warm-up calls, device events' % (MAX_STEPS, ROUNDS, STEPS, WARMUP)))
line = json.dumps(out)
print(line)
with open(OUT, 'w') as f:
    f.write(line + '\n')
