"""Ensemble beam search (decoder.EnsembleDecoder, comic_decoder_beam_ensemble) against the same number of single
Decoder.beam_search calls on ONE device in ONE process: beam 3 at the word geometry of BASELINE configs[4] (V = 25 599,
1 head, no feature-map projection, batch 50), 2 and 3 members, MAX_STEPS decode steps (default 20; random weights never
emit EOS, so every step executes).  Both sides replay their hipGraph and return the same dict (want_attention=False), are
timed in alternating rounds with device events, and the medians are reported: one JSON line.  ROUNDS (default 7), STEPS
calls per round (default 5), WARMUP (default 3)."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from comic_amd import decoder as cdec  # noqa: E402

ROUNDS, STEPS, WARMUP, MAX_STEPS = (int(os.environ.get(k, d)) for k, d in (('ROUNDS', '7'), ('STEPS', '5'), ('WARMUP', '3'),
                                                                          ('MAX_STEPS', '20')))
B, W = 50, 3
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
decs = [cdec.Decoder(spec, None, 'cuda:0', seed=k) for k in range(3)]
out = {}
for n in (2, 3):
    ens = cdec.EnsembleDecoder(decs[:n])
    steps = []

    def run_ens():
        steps.append(ens.beam_search(fm, im, W, MAX_STEPS)['step_ids'].shape[0])

    def run_singles():
        for d in decs[:n]:
            steps.append(d.beam_search(fm, im, W, MAX_STEPS, want_attention=False)['step_ids'].shape[0])
    for _ in range(WARMUP):
        run_ens()
        run_singles()
    torch.cuda.synchronize()
    t_ens, t_one = [], []
    for _ in range(ROUNDS):
        t_ens.append(timed(run_ens))
        t_one.append(timed(run_singles))
    assert set(steps) == {MAX_STEPS}, 'a decode ended early: the two sides did not run the same number of steps'
    ms_ens, ms_one = statistics.median(t_ens), statistics.median(t_one)
    out['%d members' % n] = {
        'ensemble_ms': round(ms_ens, 4), 'singles_ms': round(ms_one, 4), 'ensemble_over_singles': round(ms_ens / ms_one, 4),
        'ensemble_ms_per_member_step': round(ms_ens / n / MAX_STEPS, 4), 'single_ms_per_step': round(ms_one / n / MAX_STEPS, 4),
        'ensemble_ms_min_max': [round(min(t_ens), 4), round(max(t_ens), 4)],
        'singles_ms_min_max': [round(min(t_one), 4), round(max(t_one), 4)],
        'single_beam_path': int(decs[0].lib.comic_decoder_beam_path()),
        'ensemble_workspace_bytes': int(next(iter(ens._ctxs.values())).nbytes)}
    del ens
    torch.cuda.empty_cache()
out['config'] = ('word geometry V = 25599, B = 50, beam 3, %d steps, hipGraph replay on both sides, host post-processing of '
                 'beam_search included on both, median of %d alternating rounds of %d calls after %d warm-up calls, device events'
                 % (MAX_STEPS, ROUNDS, STEPS, WARMUP))
print(json.dumps(out))
