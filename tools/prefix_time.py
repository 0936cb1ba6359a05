"""Forced-prefix decoding (EnsembleDecoder.beam_search(prefix=), comic_decoder_beam_search_prefixed) against the SAME
executor without a prefix, on ONE device in ONE process: the word geometry of BASELINE configs[4] (V = 25 599, 1 head, no
feature-map projection, batch 50), MAX_STEPS decode steps (default 20; random weights never emit EOS, so every step
executes), one member of weight 1, a random prefix of P = 3 tokens for every image.
  beam_w3 ............ EnsembleDecoder([dec]).beam_search at beam 3: comic_decoder_beam_search, the split step in 3 launches
  beam_w3_prefix ..... the same call with BeamPrefix(table): one mask launch more in each of the first 3 steps, whose split
                       step ranks through the mask (the Bans instantiations)
  sampled_n5 ......... the same executor with BeamSampling(0.8, 3) at n = 5
  sampled_n5_prefix .. the same call with BeamPrefix(table)
All sides replay their hipGraph and return the same dict, are timed in alternating rounds with device events, and the
medians are reported, and beside them the captured loops alone (20 replays back to back) and what the host's walk for
`prefix_log_prob` takes per call (it is part of a prefixed beam_search): one JSON line, printed and written to OUT (default
profiles/r19_prefix_time.json).  ROUNDS (default 7), STEPS calls per round (default 5), WARMUP (default 3).  Not measured
here: COCO metrics of prompted captions, radix strides (a radix word is S forced steps), and prefixes beside constraints,
groups or required words."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from comic_amd import decoder as cdec  # noqa: E402

ROUNDS, STEPS, WARMUP, MAX_STEPS = (int(os.environ.get(k, d)) for k, d in (('ROUNDS', '7'), ('STEPS', '5'), ('WARMUP', '3'),
                                                                          ('MAX_STEPS', '20')))
OUT = os.environ.get('OUT', os.path.join(ROOT, 'profiles', 'r19_prefix_time.json'))
B, P = 50, 3
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
table = rng.integers(0, spec.V - 2, (B, P)).astype(np.int32)
steps, forced, last = [], {}, {}


def side(name, W, **kw):
    def run():
        r = ens.beam_search(fm, im, W, MAX_STEPS, **kw)
        steps.append(r['step_ids'].shape[0])
        if 'prefix' in kw:                                    # the best caption of every image starts with its row
            forced[name] = bool((r['predicted_ids'][:P, :, 0].T == table).all())
            last[name] = r
    return run


smp = cdec.BeamSampling(0.8, 3)
sides = {'beam_w3': side('beam_w3', 3), 'beam_w3_prefix': side('beam_w3_prefix', 3, prefix=cdec.BeamPrefix(table)),
         'sampled_n5': side('sampled_n5', 5, sampling=smp),
         'sampled_n5_prefix': side('sampled_n5_prefix', 5, sampling=smp, prefix=cdec.BeamPrefix(table))}
ctx_of = {}
for _ in range(WARMUP):
    for k, fn in sides.items():
        fn()
        ctx_of.setdefault(k, list(ens._ctxs.values())[-1])        # (a side's first call builds its context)
torch.cuda.synchronize()
assert all(forced.values()) and len(forced) == 2, 'a prefixed side did not emit its prefix'
times = {k: [] for k in sides}
for _ in range(ROUNDS):
    for k, fn in sides.items():
        times[k].append(timed(fn))
assert set(steps) == {MAX_STEPS}, 'a decode ended early: the sides did not run the same number of steps'
med = {k: statistics.median(v) for k, v in times.items()}
out = {k + '_ms': round(v, 4) for k, v in med.items()}
out.update({k + '_ms_min_max': [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})
for k in ('beam_w3', 'sampled_n5'):
    out[k + '_prefix_over_plain'] = round(med[k + '_prefix'] / med[k], 4)
    out[k + '_prefix_minus_plain_us_per_forced_step'] = round(1e3 * (med[k + '_prefix'] - med[k]) / P, 2)
# the device alone: the captured loop of every side, replayed back to back (no host work between the replays)
replay = {}
for k, ctx in ctx_of.items():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        ctx.graph.replay()
    e1.record()
    e1.synchronize()
    replay[k] = e0.elapsed_time(e1) / 20
out.update({k + '_replay_ms': round(v, 4) for k, v in replay.items()})
for k in ('beam_w3', 'sampled_n5'):
    out[k + '_prefix_minus_plain_replay_us_per_forced_step'] = round(1e3 * (replay[k + '_prefix'] - replay[k]) / P, 2)
# the host's share of the difference: prefix_log_prob walks the parents of the result (numpy, no launch)
walk = {}
for k, r in last.items():
    t0 = time.perf_counter()
    for _ in range(50):
        cdec.BeamPrefix(table).prefix_log_probs(r, 0.0, None, spec.end_id)
    walk[k] = round(1e6 * (time.perf_counter() - t0) / 50, 1)
out.update(
    host_prefix_log_prob_us=walk, contexts=len(ens._ctxs), graphs=sum(1 for c in ens._ctxs.values() if c.graph is not None),
    config=('word geometry V = 25599, B = 50, beam 3 and n = 5 samples at temperature 0.8, a random prefix of %d tokens per '
            'image, %d steps, one member, hipGraph replay on all sides, host post-processing of beam_search included, median '
            'of %d alternating rounds of %d calls after %d warm-up calls, device events' % (P, MAX_STEPS, ROUNDS, STEPS, WARMUP)),
    not_measured='COCO metrics of prompted captions; radix strides; a prefix beside constraints, groups or required words')
line = json.dumps(out)
print(line)
with open(OUT, 'w') as f:
    f.write(line + '\n')
