"""Beam search with required words (EnsembleDecoder.beam_search(required=), comic_decoder_beam_required) against the SAME
executor ungrouped and against diverse beam search with as many groups as banks and diversity 0 (the same launch count per
step), on ONE device in ONE process: the word geometry of BASELINE configs[4] (V = 25 599, 1 head, no feature-map
projection, batch 50), MAX_STEPS decode steps (default 20; random weights never emit EOS, so every step executes), one
member of weight 1, random required words (every image names all C).
  C = 2 at beam 6 (3 banks) and C = 3 at beam 8 (4 banks), one token per word:
  ungrouped_wW ... EnsembleDecoder([dec]).beam_search at beam W: comic_decoder_beam_ensemble, the split step in 3 launches
  groups_wW ...... the same call with BeamGroups(banks, 0.0): the split step in 1 + 2 banks launches
  required_wW .... the same call with BeamRequired(table): the bookkeeping launch + the split step in 1 + 2 banks launches
All sides replay their hipGraph and return the same dict, are timed in alternating rounds with device events, and the
medians are reported: one JSON line, printed and written to OUT (default profiles/r14_required_time.json).  ROUNDS
(default 7), STEPS calls per round (default 5), WARMUP (default 3)."""
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
OUT = os.environ.get('OUT', os.path.join(ROOT, 'profiles', 'r14_required_time.json'))
B, CASES = 50, ((2, 6), (3, 8))             # (required words C, beam W)
spec = cdec.DecoderSpec(V=25599, token_type='word', H=1, fm_projection=None, start_id=25597, end_id=25598)


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
steps, paths, met = [], {}, {}


def side(name, W, **kw):
    def run():
        r = ens.beam_search(fm, im, W, MAX_STEPS, **kw)
        steps.append(r['step_ids'].shape[0])
        paths[name] = int(dec.lib.comic_beam_step_ensemble_path())
        if 'met' in r:
            met[name] = float(np.mean(r['met']))
    return run


sides, launches = {}, {}
for C_, W in CASES:
    table = rng.integers(0, spec.V - 2, (B, C_, 1)).astype(np.int32)
    for name, kw, n in (('ungrouped_w%d' % W, {}, 3), ('groups_w%d' % W, dict(groups=cdec.BeamGroups(C_ + 1, 0.0)), 3 + 2 * C_),
                        ('required_w%d' % W, dict(required=cdec.BeamRequired(table)), 4 + 2 * C_)):
        sides[name], launches[name] = side(name, W, **kw), n
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
for C_, W in CASES:
    out['required_w%d_over_ungrouped' % W] = round(med['required_w%d' % W] / med['ungrouped_w%d' % W], 4)
    out['required_w%d_over_groups' % W] = round(med['required_w%d' % W] / med['groups_w%d' % W], 4)
out.update({k + '_ms_per_step': round(v / MAX_STEPS, 4) for k, v in med.items()})
out.update(
    step_launches=launches, split_form={k: paths[k] for k in sides}, mean_met=met,
    config=('word geometry V = 25599, B = 50, C = 2 at beam 6 and C = 3 at beam 8 (one token per word, random words), %d '
            'steps, one member, groups = banks at diversity 0, hipGraph replay on all sides, host post-processing of '
            'beam_search included, median of %d alternating rounds of %d calls after %d warm-up calls, device events'
            % (MAX_STEPS, ROUNDS, STEPS, WARMUP)))
line = json.dumps(out)
print(line)
with open(OUT, 'w') as f:
    f.write(line + '\n')
