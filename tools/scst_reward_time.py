"""The SCST reward on the device (comic_scst_reward) timed two ways, on ONE device in ONE process.
  (a) launch ... the reward launch alone against the host scorer on the same captions: word tokens, B = 32 images, R = 5
                 references, T = 20 steps, synthetic captions of 8 to 20 words from 200 words (n-grams do overlap, as the
                 rollouts and references of one image do), the idf table of tools/consensus_time.py (14 840 n-grams).  W = 7
                 rollouts with a greedy row, W = 5 and W = 32 with the leave-one-out baseline.  Device: the C entry called
                 LAUNCHES times back to back into outputs allocated once, device events around them.  Host:
                 captionScorer.get_hypo_scores (get_scores for leave-one-out) with 16 threads on the text of the same
                 captions, wall clock; the text conversion is not timed.  max_abs_device_minus_host: the largest
                 difference between the two rewards.
  (b) step ..... the SCST step of the benchmark's SCST geometry (bench.py: COMIC-256, radix tokens of base 256, 10 003-entry
                 vocabulary, batch 32, 7 rollouts, 5 references of 8 to 14 words) in images/s, from encoder features that
                 are given (the frozen CNN's forward is the same work in every form and is left out): rollouts -> text and
                 target ids -> the update's forward pass -> reward -> loss, backward, Adam.  Random weights with <EOS>
                 suppressed: every rollout runs all STEP_ITERS = 29 steps and nothing is cut, so the host and the device
                 forms score the same captions.  Forms: `default` (beam + greedy, host reward: the launches of the loop
                 before the options existed), `beam_device` (the same rollouts, device reward), `sample_host` and
                 `sample_device` (7 samples, leave-one-out).  `phases`: every form once more, one drained step at a time,
                 split into rollout / idle / update (device events on the one stream), reward (device events around the
                 launch, or the host scorer's wall clock), fetch and text (host).  FORMS=default runs that form alone with nothing this tool's
                 commit added: the same file times the parent commit (OUT names the other file).
Rounds alternate between the sides; every side is warmed first.  One JSON line, printed and written to OUT (default
profiles/r18_scst_reward_time.json).  ROUNDS (default 7), STEPS per round (default 5), WARMUP (default 3), LAUNCHES (50)."""
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from comic_amd import decoder as cdec, optim  # noqa: E402
from comic_amd.ops import build_radix_wtoi, id_to_caption, radix_ids_to_captions_and_ids  # noqa: E402
from comic_amd.scst.scorers import captionScorer  # noqa: E402

ROUNDS, STEPS, WARMUP, LAUNCHES, STEP_ITERS, PHASE_STEPS = (int(os.environ.get(k, d)) for k, d in (
    ('ROUNDS', '7'), ('STEPS', '5'), ('WARMUP', '3'), ('LAUNCHES', '50'), ('STEP_ITERS', '29'), ('PHASE_STEPS', '9')))
FORMS = os.environ.get('FORMS', 'default,beam_device,sample_host,sample_device').split(',')
PARTS = os.environ.get('PARTS', 'launch,step').split(',')
OUT = os.environ.get('OUT', os.path.join(ROOT, 'profiles', 'r18_scst_reward_time.json'))
DEV = 'cuda:0'
out = {}


def device_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def wall_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def alternate(sides):
    """sides: name -> (timer, fn, calls) -> name -> list of ROUNDS times; every side warmed, rounds alternating."""
    for _, fn, _ in sides.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, (timer, fn, calls) in sides.items():
            times[k].append(timer(fn, calls))
    return times


# ---- (a) the launch alone ------------------------------------------------------------------------------------------------------
if 'launch' in PARTS:
    B, R, T, V, END, WORDS, REF_LEN = 32, 5, 20, 25599, 25598, 200, 5000
    rng = np.random.default_rng(0)
    df = {}
    for _ in range(20000):
        df[tuple('w%d' % x for x in rng.integers(0, WORDS, rng.integers(1, 5)))] = float(rng.integers(1, REF_LEN))
    wtoi = {'<PAD>': -1}
    wtoi.update({'w%d' % i: i for i in range(V - 1)})
    wtoi['<EOS>'] = END
    cfg = types.SimpleNamespace(token_type='word', radix_base=0, wtoi=wtoi, itow={str(i): w for w, i in wtoi.items()})
    dfd = dict(document_frequency=df, ref_len=REF_LEN)
    scorer = captionScorer(dfd, dict(ciderD=1.0, bleu=[0, 0, 0, 2]), n_threads=16)
    lib = cdec.L.load()

    def captions(n):
        ids = rng.integers(0, WORDS, (T, B, n)).astype(np.int32)
        for b in range(B):
            for w in range(n):
                ids[rng.integers(8, T + 1):, b, w] = END
        return ids
    refs = [[' '.join('w%d' % x for x in rng.integers(0, WORDS, rng.integers(8, 21))) for _ in range(R)] for _ in range(B)]
    res = {}
    for W, base in ((7, 'greedy'), (5, 'mean'), (32, 'mean')):
        reward = cdec.Reward.from_pickle(dfd, cfg, baseline=base, weights_ciderD=1.0, weights_bleu=(0, 0, 0, 2))
        packed = cdec.RewardRefs.pack(refs, reward.vocab)
        ids = captions(W)
        greedy = captions(1)[:, :, 0].copy() if base == 'greedy' else None
        ids_d = torch.from_numpy(ids).to(DEV)
        greedy_d = torch.from_numpy(greedy).to(DEV) if greedy is not None else None
        o = cdec.scst_reward(lib, torch, ids_d, packed, reward, greedy_d)     # outputs allocated once, then the raw entry
        refs_d, n_d = packed.device(torch, DEV)
        keys, g = reward.idf.device(torch, DEV)
        v, st = reward.vocab, torch.cuda.current_stream().cuda_stream
        wb = (cdec.C.c_double * 4)(*reward.weights_bleu)

        def launch():
            rc = lib.comic_scst_reward(ids_d.data_ptr(), T, B, W, cdec.L.ptr(greedy_d), T if greedy is not None else 0, None, 0,
                                       v.end_id, 0, 1, v.n_ids, refs_d.data_ptr(), n_d.data_ptr(), R, packed.refs.shape[2],
                                       keys.data_ptr(), g.data_ptr(), reward.idf.cap, reward.idf.log_ref_len, 6.0, 1.0, wb,
                                       cdec.Reward.BASELINES[base], o['cider'].data_ptr(), o['bleu'].data_ptr(),
                                       o['reward'].data_ptr(), o['baseline'].data_ptr(), o['advantage'].data_ptr(), st)
            assert rc == 0
        sample = [[s] for s in id_to_caption(ids.transpose(2, 1, 0).reshape(W * B, T), cfg)]
        if greedy is not None:
            cap_g = [[s] for s in id_to_caption(greedy.T, cfg)]
            host = lambda: scorer.get_hypo_scores(refs, sample, cap_g)      # noqa: E731
            _, sc_s, sc_g = host()
            want = np.concatenate([sc_s.reshape(W, B).T, sc_g[:B, None]], axis=1)
        else:
            host = lambda: scorer.get_scores(refs, sample)                  # noqa: E731
            want = host().reshape(W, B).T
        agree = float(np.abs(o['reward'].cpu().numpy() - want).max())
        t = alternate({'launch': (device_ms, launch, LAUNCHES), 'host': (wall_ms, host, STEPS)})
        med = {k: statistics.median(x) for k, x in t.items()}
        res['W%d_%s' % (W, base)] = dict(
            launch_ms=round(med['launch'], 4), host_ms=round(med['host'], 4),
            launch_ms_min_max=[round(min(t['launch']), 4), round(max(t['launch']), 4)],
            host_ms_min_max=[round(min(t['host']), 4), round(max(t['host']), 4)],
            host_over_launch=round(med['host'] / med['launch'], 1), max_abs_device_minus_host=agree,
            lds_bytes=int(lib.comic_scst_reward_workspace(B, W, int(greedy is not None), T, T if greedy is not None else 0, 1,
                                                          R, packed.refs.shape[2])))
    out['launch'] = res
    out['launch_config'] = ('word tokens, B = %d, R = %d, T = %d, captions of 8..20 words from %d words, idf table of %d n-grams in '
                            '%d slots, weights CIDEr-D 1 + BLEU-4 2; launch: %d calls of the C entry back to back, device events; '
                            'host: captionScorer, 16 threads, wall clock, %d calls; median of %d alternating rounds after %d '
                            'warm-up calls' % (B, R, T, WORDS, reward.idf.kept, reward.idf.cap, LAUNCHES, STEPS, ROUNDS, WARMUP))

# ---- (b) the SCST step ----------------------------------------------------------------------------------------------------------
if 'step' in PARTS:
    from comic_amd.scst import prepro_ngrams
    Bs, W = 32, 7
    rng = np.random.default_rng(7)
    words = ['w%d' % i for i in range(10000)]
    wtoi = {'<PAD>': -1}
    for i, w in enumerate(words):
        wtoi[w] = i
    for tok in ('<UNK>', '<GO>', '<EOS>'):
        wtoi[tok] = len(wtoi) - 1
    cfg = types.SimpleNamespace(token_type='radix', radix_base=256, wtoi=wtoi, itow={str(v): k for k, v in wtoi.items()},
                                scst_weight_ciderD=1.0, scst_weight_bleu=[0, 0, 0, 2])
    table = build_radix_wtoi(wtoi, 256)
    refs = [[' '.join(rng.choice(words[:200], int(rng.integers(8, 15)))) for _ in range(5)] for _ in range(Bs)]
    df = prepro_ngrams.build(['i%d,<GO> %s <EOS>' % (i, r) for i, rl in enumerate(refs) for r in rl])
    scorer = captionScorer(df, dict(ciderD=1.0, bleu=[0, 0, 0, 2]))
    spec = cdec.DecoderSpec()
    dec = cdec.Decoder(spec, None, DEV, seed=4)
    dec.params.view('b_o')[257] = -30.0
    opt = optim.AdamTF(dec.params)
    fm = torch.from_numpy(rng.standard_normal((Bs, spec.M, spec.C)).astype(np.float32)).to(DEV)
    im = torch.from_numpy(rng.standard_normal((Bs, spec.Cg)).astype(np.float32)).to(DEV)
    fm_w, im_w = fm.repeat(W, 1, 1), im.repeat(W, 1)
    count = [0]

    class Probe:
        """Per-phase times of one step, when `on`: device events by name, host wall clock by name (ms)."""
        on = False

        def __init__(self):
            self.ev, self.host = {}, {}

        def mark(self, name, stream=None):
            if self.on:
                e = torch.cuda.Event(enable_timing=True)
                e.record(stream or torch.cuda.current_stream())
                self.ev[name] = e

        def timed(self, name, fn):
            if not self.on:
                return fn()
            t0 = time.perf_counter()
            r = fn()
            self.host[name] = self.host.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
            return r
    pr = Probe()

    def update(ids, rewards):
        res = dec.train_step(None, None, ids, rewards=rewards, training=True, use_graph=True, phase='bwd')
        opt.step(dec.grads, 1e-3)
        pr.mark('u1')
        return res

    def forward(ids):
        pr.mark('u0')
        dec.train_step(fm_w, im_w, ids, training=True, use_graph=True, phase='fwd')

    def default():
        pr.mark('r0')
        fetch_beam = dec.beam_search_ids(fm, im, W, STEP_ITERS)
        fetch_greedy = dec.greedy(fm, im, STEP_ITERS, defer=True)
        pr.mark('r1')
        beam = pr.timed('fetch', fetch_beam).transpose(2, 1, 0)
        caps, ids = pr.timed('text', lambda: radix_ids_to_captions_and_ids(beam.reshape(-1, beam.shape[-1]), cfg, table))
        cap_beam = [[c] for c in caps]
        forward(ids)
        greedy = pr.timed('fetch', fetch_greedy)[0]
        cap_greedy = pr.timed('text', lambda: [[c] for c in id_to_caption(greedy, cfg)])
        _, sc_s, sc_g = pr.timed('reward', lambda: scorer.get_hypo_scores(refs, cap_beam, cap_greedy))
        return update(ids, (sc_s - sc_g).astype(np.float32))
    forms = {'default': default}
    if set(FORMS) - {'default'}:
        from comic_amd.ops import captions_to_batched_ids
        from comic_amd.train_fn import leave_one_out
        rw = {b: cdec.Reward.from_pickle(df, cfg, baseline=b) for b in ('greedy', 'mean')}
        packed = cdec.RewardRefs.pack(refs, rw['mean'].vocab)        # (uploaded once: the tool's batch never changes)
        packed_g = cdec.RewardRefs.pack(refs, rw['greedy'].vocab)

        def launch(ids_device, refs_packed, reward, greedy_ids=None, greedy_eos=None):
            pr.mark('q0')
            res = dec.scst_reward(ids_device, refs_packed, reward, greedy_ids, greedy_eos)
            pr.mark('q1')
            return res

        def beam_device():
            pr.mark('r0')
            fetch_beam = dec.beam_search_ids(fm, im, W, STEP_ITERS)
            fetch_greedy = dec.greedy(fm, im, STEP_ITERS, defer=True)
            pr.mark('r1')
            adv = launch(fetch_beam.ids_device, packed_g, rw['greedy'], fetch_greedy.ids_device,
                         fetch_greedy.first_eos_device)['advantage']
            beam = pr.timed('fetch', fetch_beam).transpose(2, 1, 0)
            caps, ids = pr.timed('text', lambda: radix_ids_to_captions_and_ids(beam.reshape(-1, beam.shape[-1]), cfg, table))
            forward(ids)
            return update(ids, adv.reshape(-1))

        def sampled(device):
            count[0] += 1
            pr.mark('r0')
            fetch = dec.beam_search_ids(fm, im, W, STEP_ITERS, sampling=cdec.BeamSampling(1.0, 1), image_base=count[0] * Bs)
            pr.mark('r1')
            adv = launch(fetch.ids_device, packed, rw['mean'])['advantage'] if device else None
            beam = pr.timed('fetch', fetch).transpose(2, 1, 0)

            def text():
                caps = [[c] for c in id_to_caption(beam.reshape(-1, beam.shape[-1]), cfg, skip_unmapped=True)]
                return caps, captions_to_batched_ids(caps, cfg, table)
            cap_beam, ids = pr.timed('text', text)
            forward(ids)
            if device:
                return update(ids, adv.reshape(-1))
            sc = pr.timed('reward', lambda: scorer.get_scores(refs, cap_beam))
            return update(ids, leave_one_out(sc, W)[0].astype(np.float32))
        forms.update(beam_device=beam_device, sample_host=lambda: sampled(False), sample_device=lambda: sampled(True))
    forms = {k: forms[k] for k in FORMS}
    t = alternate({k: (wall_ms, fn, STEPS) for k, fn in forms.items()})
    res = {}
    for k, x in t.items():
        ips = sorted(Bs * 1e3 / v for v in x)
        res[k] = dict(images_per_sec=round(statistics.median(ips), 1), min_max=[round(ips[0], 1), round(ips[-1], 1)],
                      spread=round((ips[-1] - ips[0]) / statistics.median(ips), 4), step_ms=round(statistics.median(x), 3))
    out['step'] = res
    # where a step's time goes: every form once more with the probe on, one drained step at a time
    pr.on = True
    phases = {}
    for k, fn in forms.items():
        rows = []
        for _ in range(PHASE_STEPS):
            pr.ev, pr.host = {}, {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            e, row = pr.ev, dict(pr.host)
            row.update(step=(time.perf_counter() - t0) * 1e3, rollout=e['r0'].elapsed_time(e['r1']),
                       idle=e['r1'].elapsed_time(e['u0']), update=e['u0'].elapsed_time(e['u1']))
            if 'q0' in e:
                row['reward'] = e['q0'].elapsed_time(e['q1'])
            rows.append(row)
        phases[k] = {n + '_ms': round(statistics.median(r[n] for r in rows), 4) for n in rows[0]}
        phases[k]['reward_on'] = 'device events' if 'q0' in pr.ev else 'host, wall clock'
    pr.on = False
    out['phases'] = phases
    out['phases_config'] = ('median of %d drained steps per form.  rollout / update: device events on the main stream around the '
                            'rollout launches and around forward + loss + backward + Adam; idle: the main stream between the '
                            'two (the reward launch of the device forms lies in it); reward: device events around the launch, or the '
                            'host scorer\'s wall clock; fetch: the host\'s waits for the ids; text: ids -> text -> target ids '
                            'on the host' % PHASE_STEPS)
    out['step_config'] = ('COMIC-256 decoder, radix base 256, batch %d, %d rollouts of %d steps (<EOS> suppressed), 5 references, '
                          'reward CIDEr-D 1 + BLEU-4 2, given encoder features (no CNN forward), hipGraph replay of rollouts and '
                          'update, host scorer with %d threads; wall clock over %d steps; median and min / max of %d alternating '
                          'rounds after %d warm-up steps; spread = (max - min) / median'
                          % (Bs, W, STEP_ITERS, scorer.n_threads, STEPS, ROUNDS, WARMUP))

line = json.dumps(out)
print(line)
with open(OUT, 'w') as f:
    f.write(line + '\n')
