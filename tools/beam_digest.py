"""Bit digests of beam search (comic_decoder_beam, comic_decoder_beam_ensemble) and of the raw beam-step operators, through
the Python Decoder / EnsembleDecoder API and ctypes only -- the same file runs against any build of the library
(COMIC_HIP_LIB=<other libcomic_hip.so>), and two builds that compute the same bits print the same lines.
   python tools/beam_digest.py
Decoders: the smallest geometry of tests/test_gpu_path.py (V = 258) and the same with V = 9001, batch 4, beam 3, MAX_STEPS
steps, under the default switches, COMIC_BEAM_LOGITS=0, COMIC_FUSED_STEP=0 and length_penalty_weight = 0.7; a 2-member
ensemble at both vocabularies with and without the penalty.  Every decode runs eagerly and then as a replayed hipGraph; one
sha256 per run over step_ids, parent_ids, scores and lengths up to steps_executed, and over log_probs where the result has them.
Option decodes, at both vocabularies with batch 4 and beam 4, through the keyword API alone: constraints (min_length 4,
no_repeat_ngram 2), two groups at diversity 0.5, sampling (temperature 0.8, seed 2), sampling under top_k 5 / top_p 0.9, one
required word per image, and a 2-member ensemble with the constraints and the sampling together.
Step operators: comic_beam_step (one-member cases) and comic_beam_step_ensemble with and without its workspace on the
inputs of tests/test_gpu_ensemble.py's STEP_CASES; one sha256 over word, parent, scores, log_probs, finished, lengths.
comic_beam_step_dense at (B, W, V, D) = (4, 3, 3100, 96), (4, 5, 2500, 96), (4, 9, 2500, 96): GEMM + the single-member
split step with 16 and 40 register slots and in its rescanning form; the same six arrays."""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import comic_amd._lib as L  # noqa: E402
from comic_amd import decoder as cdec  # noqa: E402
from tests.test_gpu_ensemble import STEP_CASES, step_case  # noqa: E402

DEV = 'cuda:0'
BASE = dict(D=128, E=64, C=192, Cg=192, H=8, M=25)                 # tests/test_gpu_path.py: _spec_and_cfg
B, W, MAX_STEPS = 4, 3, 10
OPTION_W = 4                                                        # the option decodes: two groups, two banks
SWITCHES = [('default', {}, 0.0), ('no_beam_logits', {'COMIC_BEAM_LOGITS': '0'}, 0.0),
            ('no_fused_step', {'COMIC_FUSED_STEP': '0'}, 0.0), ('length_penalty', {}, 0.7)]


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def decode_digests(search, path):
    """search(use_graph) -> the beam_search dict; eager, then capture and replay."""
    out = []
    for name, use_graph in (('eager', False), ('capture', True), ('replay', True)):
        r = search(use_graph)
        if name != 'capture':
            keys = ('step_ids', 'parent_ids', 'scores', 'lengths') + (('log_probs',) if 'log_probs' in r else ())
            out.append('%s T=%d %s' % (name, r['step_ids'].shape[0], sha(r[k] for k in keys)))
    return 'path %s %s' % (path(), ' '.join(out))


def decoders():
    rng = np.random.default_rng(0)
    fm = torch.from_numpy(rng.standard_normal((B, BASE['M'], BASE['C'])).astype(np.float32)).to(DEV)
    im = torch.from_numpy(rng.standard_normal((B, BASE['Cg'])).astype(np.float32)).to(DEV)
    for V in (258, 9001):
        spec = cdec.DecoderSpec(V=V, **BASE)
        for name, env, lpw in SWITCHES:
            os.environ.update(env)
            try:
                dec = cdec.Decoder(spec, None, DEV, seed=3)        # a context (and a graph) of its own per switch
                line = decode_digests(lambda g: dec.beam_search(fm, im, W, MAX_STEPS, want_attention=False, use_graph=g,
                                                                length_penalty_weight=lpw),
                                      lambda: int(dec.lib.comic_decoder_beam_path()))
            finally:
                for k in env:
                    del os.environ[k]
            print('decoder V=%d %s %s' % (V, name, line), flush=True)
        ens = cdec.EnsembleDecoder([cdec.Decoder(spec, None, DEV, seed=3), cdec.Decoder(spec, None, DEV, seed=4)], [0.6, 0.4])
        for lpw in (0.0, 0.7):
            line = decode_digests(lambda g: ens.beam_search(fm, im, W, MAX_STEPS, use_graph=g, length_penalty_weight=lpw),
                                  lambda: int(ens.lib.comic_beam_step_ensemble_path()))
            print('ensemble V=%d lpw=%.1f %s' % (V, lpw, line), flush=True)
        cons, smp = cdec.BeamConstraints(min_length=4, no_repeat_ngram=2), cdec.BeamSampling(0.8, 2)
        rqd = cdec.BeamRequired(np.arange(5, 5 + B, dtype=np.int32).reshape(B, 1, 1))
        dec = cdec.Decoder(spec, None, DEV, seed=3)
        for name, search, kw in (('constraints', dec, dict(constraints=cons)), ('groups', dec, dict(groups=cdec.BeamGroups(2, 0.5))),
                                 ('sampling', dec, dict(sampling=smp)),
                                 ('truncation', dec, dict(sampling=smp, truncation=cdec.BeamTruncation(5, 0.9))),
                                 ('required', dec, dict(required=rqd)),
                                 ('ensemble_constraints_sampling', ens, dict(constraints=cons, sampling=smp))):
            line = decode_digests(lambda g: search.beam_search(fm, im, OPTION_W, MAX_STEPS, want_attention=False, use_graph=g, **kw),
                                  lambda: int(ens.lib.comic_beam_step_ensemble_path()))
            print('options V=%d %s %s' % (V, name, line), flush=True)


def step(c, lpw, form):
    """form: 'single' (comic_beam_step), 'ens' (ensemble, null workspace), 'ens_ws' (ensemble with its workspace)"""
    lib = L.load()
    n, Bs, Ws, V = c['logits'].shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)     # noqa: E731
    lg, lp, fin, ln = t(c['logits']), t(c['log_probs']), t(c['finished']), t(c['lengths'])
    word = torch.full((Bs, Ws), -1, dtype=torch.int32, device=DEV)
    parent = torch.full((Bs, Ws), -1, dtype=torch.int32, device=DEV)
    scores = torch.zeros((Bs, Ws), dtype=torch.float32, device=DEV)
    if form == 'single':
        L.check(lib.comic_beam_step(lg.data_ptr(), lp.data_ptr(), fin.data_ptr(), ln.data_ptr(), word.data_ptr(),
                                    parent.data_ptr(), scores.data_ptr(), Bs, Ws, V, c['end_id'], L.stream_ptr()), 'beam_step')
    else:
        nbytes = int(lib.comic_beam_step_ensemble_workspace(n, Bs, Ws, V)) if form == 'ens_ws' else 0
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
        wt = (C.c_float * n)(*[float(w) for w in c['wts']])
        L.check(lib.comic_beam_step_ensemble(lg.data_ptr(), wt, n, lp.data_ptr(), fin.data_ptr(), ln.data_ptr(), word.data_ptr(),
                                             parent.data_ptr(), scores.data_ptr(), Bs, Ws, V, c['end_id'], float(lpw),
                                             ws.data_ptr() if nbytes else None, nbytes, L.stream_ptr()), 'beam_step_ensemble')
    torch.cuda.synchronize()
    return sha(x.cpu().numpy() for x in (word, parent, scores, lp, fin, ln))


def steps():
    for shape, state, lpw in STEP_CASES:
        c = step_case(shape, state, lpw)
        forms = ['ens', 'ens_ws'] + (['single'] if shape[0] == 1 and lpw == 0.0 else [])
        print('step n=%d B=%d W=%d V=%d %s lpw=%.1f %s' % (shape + (state, lpw, ' '.join('%s %s' % (f, step(c, lpw, f)) for f in forms))),
              flush=True)


def dense():
    lib = L.load()
    for Bs, Ws, V, D in ((4, 3, 3100, 96), (4, 5, 2500, 96), (4, 9, 2500, 96)):
        rng = np.random.default_rng(V + Ws)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)     # noqa: E731
        y, Wo = t(rng.standard_normal((Bs * Ws, D)).astype(np.float32)), t((rng.standard_normal((D, V)) / np.sqrt(D)).astype(np.float32))
        bo = t((0.1 * rng.standard_normal(V)).astype(np.float32))
        lp = t(-rng.uniform(0.0, 3.0, (Bs, Ws)).astype(np.float32))
        fin = np.zeros((Bs, Ws), np.int32)
        fin[1, 1] = 1
        fin, ln = t(fin), t(rng.integers(0, 5, (Bs, Ws)).astype(np.int64))
        word = torch.full((Bs, Ws), -1, dtype=torch.int32, device=DEV)
        parent = torch.full((Bs, Ws), -1, dtype=torch.int32, device=DEV)
        scores = torch.zeros((Bs, Ws), dtype=torch.float32, device=DEV)
        nb = int(lib.comic_beam_step_dense_workspace(Bs, Ws, D, V))
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        L.check(lib.comic_beam_step_dense(y.data_ptr(), Wo.data_ptr(), bo.data_ptr(), lp.data_ptr(), fin.data_ptr(), ln.data_ptr(),
                                          word.data_ptr(), parent.data_ptr(), scores.data_ptr(), Bs, Ws, D, V, V - 1, ws.data_ptr(), nb,
                                          L.stream_ptr()), 'beam_step_dense')
        torch.cuda.synchronize()
        print('dense B=%d W=%d V=%d D=%d %s' % (Bs, Ws, V, D, sha(x.cpu().numpy() for x in (word, parent, scores, lp, fin, ln))),
              flush=True)


if __name__ == '__main__':
    decoders()
    steps()
    dense()
