"""Consensus selection (comic_caption_consensus) timed three ways, on ONE device in ONE process, at the word geometry of the
other decode timings (V = 25 599, 1 head, no feature-map projection, batch 50, MAX_STEPS = 20 steps; random weights never
emit EOS, so every step executes), for n = 5 and n = 32 samples per image:
  launch ..... the consensus launch alone, on the device ids of a sampled decode: the C entry called LAUNCHES times (default
               50) back to back into outputs allocated once, device events around them (a call through
               Decoder.consensus allocates its outputs and is bound by the host)
  share ...... that time over the sampled decode it follows (EnsembleDecoder.beam_search(sampling=), hipGraph replay, host
               post-processing included), and the same decode with consensus= against the one without
  host ....... the path a user has without it: id_to_caption on all B * n samples, then the host scorer
               (captionScorer._score with 16 threads, each sample's siblings as its references; CIDEr-D is what is read,
               the entry forms BLEU alongside), wall clock
Two sets of ids: `decoded`, the decode's own samples (random weights: 20 tokens that hardly ever repeat, so every search
of a sibling's n-grams runs to its end), and `overlap`, synthetic captions of 8 to 20 words from 200 words (n-grams do
overlap, as real samples of one image do).  The idf table and the host scorer are built from one synthetic df dict.  The
tool also reports the largest |device utility - host CIDEr-D| it saw: the two paths compute the same number.
One JSON line, printed and written to OUT (default profiles/r17_consensus_time.json).  ROUNDS (default 7), STEPS calls per
round (default 5), WARMUP (default 3), LAUNCHES (default 50)."""
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
from comic_amd.ops import id_to_caption  # noqa: E402
from comic_amd.scst.scorers import captionScorer  # noqa: E402

ROUNDS, STEPS, WARMUP, MAX_STEPS, LAUNCHES = (int(os.environ.get(k, d)) for k, d in (
    ('ROUNDS', '7'), ('STEPS', '5'), ('WARMUP', '3'), ('MAX_STEPS', '20'), ('LAUNCHES', '50')))
OUT = os.environ.get('OUT', os.path.join(ROOT, 'profiles', 'r17_consensus_time.json'))
B, TEMP, V, END, WORDS, REF_LEN = 50, 0.7, 25599, 25598, 200, 5000
spec = cdec.DecoderSpec(V=V, token_type='word', H=1, fm_projection=None, start_id=25597, end_id=END)
cfg = type('Cfg', (), dict(token_type='word', wtoi={'<EOS>': END}, itow={str(i): 'w%d' % i for i in range(V)}))()

rng = np.random.default_rng(0)
df = {}
for _ in range(20000):
    df[tuple('w%d' % x for x in rng.integers(0, WORDS, rng.integers(1, 5)))] = float(rng.integers(1, REF_LEN))
idf = cdec.NgramIdf.from_document_frequency(df, REF_LEN, {'w%d' % i: [i] for i in range(V)}, 1)
cons = cdec.Consensus('uniform', 1, idf)
scorer = captionScorer(dict(document_frequency=df, ref_len=REF_LEN), dict(ciderD=1.0), n_threads=16)

fm = torch.from_numpy(rng.standard_normal((B, spec.M, spec.C)).astype(np.float32)).to('cuda:0')
im = torch.from_numpy(rng.standard_normal((B, spec.Cg)).astype(np.float32)).to('cuda:0')
dec = cdec.Decoder(spec, None, 'cuda:0', seed=0)
ens = cdec.EnsembleDecoder([dec])


def device_ms(fn, calls=STEPS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def launches_ms(fn):
    return device_ms(fn, LAUNCHES)


def raw_launch(ids):
    """The C entry on the device ids [T, B, n], outputs allocated once."""
    T, _, n = ids.shape
    util = torch.empty((B, n), dtype=torch.float64, device='cuda:0')
    best = torch.empty(B, dtype=torch.int32, device='cuda:0')
    keys, g = idf.device(torch, ids.device)
    stream = torch.cuda.current_stream().cuda_stream

    def run():
        rc = dec.lib.comic_caption_consensus(ids.data_ptr(), T, B, n, END, 1, None, 0, keys.data_ptr(), g.data_ptr(), idf.cap,
                                             idf.log_ref_len, cons.sigma, util.data_ptr(), best.data_ptr(), None, 0, stream)
        assert rc == 0
    return run


def host_ms(fn):
    t0 = time.perf_counter()
    for _ in range(STEPS):
        fn()
    return (time.perf_counter() - t0) * 1e3 / STEPS


def overlap_ids(n):
    ids = rng.integers(0, WORDS, (MAX_STEPS, B, n)).astype(np.int32)
    for b in range(B):
        for w in range(n):
            ids[rng.integers(8, MAX_STEPS + 1):, b, w] = END
    return ids


def host_path(ids):
    n = ids.shape[2]
    caps = id_to_caption(ids.transpose(1, 2, 0).reshape(B * n, -1), cfg)
    refs = [[caps[(k // n) * n + j] for j in range(n) if j != k % n] for k in range(B * n)]
    return scorer._score(caps, refs)[0].reshape(B, n)


out, seeds = {}, [0]
for n in (5, 32):
    def decode(**kw):
        seeds[0] += 1
        return ens.beam_search(fm, im, n, MAX_STEPS, sampling=cdec.BeamSampling(TEMP, seeds[0]), **kw)
    res = decode(consensus=cons)
    assert res['step_ids'].shape[0] == MAX_STEPS
    sets = dict(decoded=res['predicted_ids'], overlap=overlap_ids(n))
    dev_ids = {k: torch.from_numpy(np.ascontiguousarray(v)).to('cuda:0') for k, v in sets.items()}
    sides = {'decode': (device_ms, decode), 'decode_consensus': (device_ms, lambda: decode(consensus=cons))}
    agree = 0.0
    for k in sets:
        sides['launch_' + k] = (launches_ms, raw_launch(dev_ids[k]))
        sides['host_' + k] = (host_ms, lambda k=k: host_path(sets[k]))
        u = cdec.caption_consensus(dec.lib, torch, dev_ids[k], END, cons)[0].cpu().numpy()
        agree = max(agree, float(np.abs(u - host_path(sets[k])).max()))
    for _ in range(WARMUP):
        for _, fn in sides.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, (timer, fn) in sides.items():
            times[k].append(timer(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    r = {k + '_ms': round(v, 4) for k, v in med.items()}
    r.update({k + '_ms_min_max': [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})
    r.update(launch_share_of_decode=round(med['launch_decoded'] / med['decode'], 5),
             decode_consensus_over_decode=round(med['decode_consensus'] / med['decode'], 4),
             host_over_launch_decoded=round(med['host_decoded'] / med['launch_decoded'], 1),
             host_over_launch_overlap=round(med['host_overlap'] / med['launch_overlap'], 1),
             max_abs_device_minus_host=agree)
    out['n%d' % n] = r
out['config'] = ('word geometry V = 25599, B = 50, %d steps, one member, temperature 0.7, idf table of %d n-grams in %d slots; '
                 'decode: hipGraph replay with the host post-processing of beam_search; launch: %d calls of the C entry back to back; '
                 'host: id_to_caption + captionScorer._score, 16 threads, wall clock; median of %d alternating rounds of %d '
                 'calls after %d warm-up calls' % (MAX_STEPS, idf.kept, idf.cap, LAUNCHES, ROUNDS, STEPS, WARMUP))
line = json.dumps(out)
print(line)
with open(OUT, 'w') as f:
    f.write(line + '\n')
