"""Host time per call of the Decoder entry points that replay a hipGraph: what the Python side of comic_amd/decoder.py costs
between the caller and the graph launch.  COMIC-256 geometry, B = 64, T = T' = 20, use_graph=True.  Per call the clock
(time.perf_counter) runs around the call alone and the device is synchronised outside it; the median of CALLS (200) calls
after WARMUP (10) is reported, in microseconds, for
  train_step            one whole XE training step (device-generated dropout masks)
  train_step_fwd_bwd    the phase='fwd' + phase='bwd' pair with host rewards (both calls inside the clock)
  score                 Decoder.score
  beam_search_ids       the enqueue part of beam_search_ids at beam 3 (the fetch is outside the clock)
   python tools/decoder_host_time.py [NAME=TREE ...]
Every TREE (a checkout of this repository; default: this=<the one this file is in>) is measured in a fresh process of its
own, one after the other, against ONE build of the library (COMIC_HIP_LIB, default this checkout's): one JSON object with
one entry per NAME, in the order given.  A tree named twice (a=DIR b=DIR) shows the run-to-run spread."""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
CALLS, WARMUP = (int(os.environ.get(k, d)) for k, d in (('CALLS', '200'), ('WARMUP', '10')))
B, L_CAP, BEAM, MAX_STEPS = 64, 21, 3, 20


def measure(tree):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from comic_amd import decoder as cdec

    spec = cdec.DecoderSpec()
    rng = np.random.default_rng(0)
    fm = torch.from_numpy(rng.standard_normal((B, spec.M, spec.C)).astype(np.float32)).to('cuda:0')
    im = torch.from_numpy(rng.standard_normal((B, spec.Cg)).astype(np.float32)).to('cuda:0')
    caps = np.full((B, L_CAP), -1, np.int64)
    for b in range(B):
        n = L_CAP - 2 if b == 0 else 6 + b % 13
        caps[b, 0], caps[b, 1:1 + n], caps[b, 1 + n] = spec.start_id, rng.integers(0, min(spec.V - 2, 256), n), spec.end_id
    rewards = rng.standard_normal(B).astype(np.float32)

    def pair(dec):
        dec.train_step(fm, im, caps, training=True, use_graph=True, phase='fwd')
        dec.train_step(None, None, caps, rewards=rewards, training=True, use_graph=True, phase='bwd')

    def ids(dec):
        return dec.beam_search_ids(fm, im, BEAM, MAX_STEPS, use_graph=True)
    calls = dict(train_step=lambda dec: dec.train_step(fm, im, caps, training=True, use_graph=True), train_step_fwd_bwd=pair,
                 score=lambda dec: dec.score(fm, im, caps, use_graph=True), beam_search_ids=ids)
    out = {}
    for name, call in calls.items():
        dec = cdec.Decoder(spec, None, 'cuda:0')        # a decoder, and so its contexts and graphs, per entry point
        us = []
        for i in range(WARMUP + CALLS):
            t0 = time.perf_counter()
            r = call(dec)
            t1 = time.perf_counter()
            if name == 'beam_search_ids':
                r()
            torch.cuda.synchronize()
            if i >= WARMUP:
                us.append((t1 - t0) * 1e6)
        ctxs = getattr(dec, {'score': '_score_ctxs', 'beam_search_ids': '_infer_ctxs'}.get(name, '_ctx'))
        assert all(c.graph is not None or name == 'train_step_fwd_bwd' for c in ctxs.values()), name
        us.sort()
        out[name] = {'median_us': round(statistics.median(us), 2), 'p10_us': round(us[len(us) // 10], 2),
                     'p90_us': round(us[len(us) * 9 // 10], 2)}
        del dec
        torch.cuda.empty_cache()
    return out


def main(args):
    if args[:1] == ['--one']:
        print(json.dumps(measure(args[1])))
        return
    root = os.path.dirname(HERE)
    env = dict(os.environ)
    env.setdefault('COMIC_HIP_LIB', os.path.join(root, 'comic-compact-image-captioning-with-attention_amd', 'lib',
                                                 'libcomic_hip.so'))
    out = {'config': 'COMIC-256, B = %d, T = %d, beam %d, use_graph=True; perf_counter around the call alone, synchronised '
                     'outside it; %d calls after %d warm-up calls' % (B, L_CAP - 1, BEAM, CALLS, WARMUP)}
    for arg in args or ['this=' + root]:
        name, tree = arg.split('=', 1)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--one', os.path.abspath(tree)], env=env,
                           stdout=subprocess.PIPE, check=True, timeout=600)
        out[name] = json.loads(p.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main(sys.argv[1:])
