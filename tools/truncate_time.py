"""Top-k / nucleus truncation of the sampled step (EnsembleDecoder.beam_search(sampling=, truncation=),
comic_decoder_beam_truncated) against the SAME executor's untruncated sampling (comic_decoder_beam_sampled, the path this
work leaves as it was), on ONE device in ONE process: n = 5 samples per image at the word geometry of BASELINE configs[4]
(V = 25 599, 1 head, no feature-map projection, batch 50), MAX_STEPS decode steps (default 20; random weights never emit
EOS, so every step executes), one member of weight 1, temperature 0.7.
  sampled ..... BeamSampling(0.7, seed) alone: the split step in 3 launches
  top_k_40 .... the same call with BeamTruncation(top_k=40): one more launch per step, 250 workgroups of 1024 threads
  top_p_0.9 ... with BeamTruncation(top_p=0.9)
  both ........ with BeamTruncation(40, 0.9)
A new seed every call (the seed words are written in front of every replay).  All sides replay their hipGraph and return
the same dict, are timed in alternating rounds with device events, and the medians are reported, with the cost of the
truncation per step: (side - sampled) / MAX_STEPS.
One JSON line, printed and written to OUT (default profiles/r13_truncate_time.json).  ROUNDS (default 7), STEPS calls per
round (default 5), WARMUP (default 3)."""
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
OUT = os.environ.get('OUT', os.path.join(ROOT, 'profiles', 'r13_truncate_time.json'))
B, W, TEMP = 50, 5, 0.7
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
steps, calls = [], [0]


def side(truncation):
    def run():
        calls[0] += 1
        steps.append(ens.beam_search(fm, im, W, MAX_STEPS, sampling=cdec.BeamSampling(TEMP, calls[0]),
                                     truncation=truncation)['step_ids'].shape[0])
    return run


sides = {'sampled': side(None), 'top_k_40': side(cdec.BeamTruncation(top_k=40)), 'top_p_0.9': side(cdec.BeamTruncation(top_p=0.9)),
         'both': side(cdec.BeamTruncation(40, 0.9))}
for _ in range(WARMUP):
    for fn in sides.values():
        fn()
torch.cuda.synchronize()
times = {k: [] for k in sides}
for _ in range(ROUNDS):
    for k, fn in sides.items():
        times[k].append(timed(fn))
assert set(steps) == {MAX_STEPS}, 'a decode ended early: the sides did not run the same number of steps'
assert len(ens._ctxs) == 4 and all(c.graph is not None for c in ens._ctxs.values()), 'a side did not replay one graph'
med = {k: statistics.median(v) for k, v in times.items()}
out = {k + '_ms': round(v, 4) for k, v in med.items()}
out.update({k + '_ms_min_max': [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})
for k in ('top_k_40', 'top_p_0.9', 'both'):
    out[k + '_over_sampled'] = round(med[k] / med['sampled'], 4)
    out[k + '_truncate_ms_per_step'] = round((med[k] - med['sampled']) / MAX_STEPS, 4)
out.update(
    sampled_ms_per_step=round(med['sampled'] / MAX_STEPS, 4),
    config=('word geometry V = 25599, B = 50, n = beam = 5, %d steps, one member, temperature 0.7, hipGraph replay on all '
            'sides, host post-processing of beam_search included, median of %d alternating rounds of %d calls after %d '
            'warm-up calls, device events' % (MAX_STEPS, ROUNDS, STEPS, WARMUP)))
line = json.dumps(out)
print(line)
with open(OUT, 'w') as f:
    f.write(line + '\n')
