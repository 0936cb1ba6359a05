"""Diverse beam search (EnsembleDecoder.beam_search(groups=), comic_decoder_beam_diverse) against the SAME executor
ungrouped, on ONE device in ONE process: beam 6 at the word geometry of BASELINE configs[4] (V = 25 599, 1 head, no
feature-map projection, batch 50), MAX_STEPS decode steps (default 20; random weights never emit EOS, so every step
executes), one member of weight 1.
  ungrouped ... EnsembleDecoder([dec]).beam_search at beam 6: comic_decoder_beam_ensemble, the split step in 3 launches
  groups_G .... the same call with BeamGroups(G, 0.5), G = 2, 3, 6: the split step in 1 + 2 G launches
All sides replay their hipGraph and return the same dict, are timed in alternating rounds with device events, and the
medians are reported: one JSON line, printed and written to OUT (default profiles/r11_diverse_time.json).  ROUNDS
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
OUT = os.environ.get('OUT', os.path.join(ROOT, 'profiles', 'r11_diverse_time.json'))
B, W, LAM, GROUPS = 50, 6, 0.5, (2, 3, 6)
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
steps, paths = [], {}


def side(name, groups):
    def run():
        steps.append(ens.beam_search(fm, im, W, MAX_STEPS, groups=groups)['step_ids'].shape[0])
        paths[name] = int(dec.lib.comic_beam_step_ensemble_path())
    return run


sides = {'ungrouped': side('ungrouped', None)}
sides.update({'groups_%d' % G: side('groups_%d' % G, cdec.BeamGroups(G, LAM)) for G in GROUPS})
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
out.update({'groups_%d_over_ungrouped' % G: round(med['groups_%d' % G] / med['ungrouped'], 4) for G in GROUPS})
out.update({k + '_ms_per_step': round(v / MAX_STEPS, 4) for k, v in med.items()})
out.update(
    step_launches={k: (3 if k == 'ungrouped' else 1 + 2 * int(k.split('_')[1])) for k in sides},
    split_form={k: paths[k] for k in sides},
    config=('word geometry V = 25599, B = 50, beam 6, %d steps, one member, diversity 0.5, hipGraph replay on all sides, host '
            'post-processing of beam_search included, median of %d alternating rounds of %d calls after %d warm-up calls, '
            'device events' % (MAX_STEPS, ROUNDS, STEPS, WARMUP)))
line = json.dumps(out)
print(line)
with open(OUT, 'w') as f:
    f.write(line + '\n')
